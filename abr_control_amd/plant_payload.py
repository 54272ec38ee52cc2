"""The rigid-body plant carrying a payload that differs from row to row (include/abrk.h,
abrk_forward_dynamics_payload_batch / abrk_plant_step_payload_batch): engine.forward_dynamics and engine.plant_step with
one more array, `payload` [B,4] = m, rx, ry, rz - a point mass m >= 0 at offset r from the origin of the end-effector
frame, in that frame's coordinates (the x of robot_config.Tx("EE", q, x=r)).  It changes M, C and g of that row's PLANT;
the controllers keep the robot_config's model.  The engine's own two functions keep their signatures (callers pass their
arguments positionally); with payload None the functions here make exactly the engine's calls."""
import ctypes as C

import numpy as np

from . import engine
from ._lib import check


def forward_dynamics(arm_id, n, q, dq, u, ddq=None, dtype=np.float64, device=0, stream=None, effects=None,
                     tau_ext=None, wrench=None, payload=None):
    """engine.forward_dynamics for rows that carry `payload` [B,4]: ddq = (M + m Jp^T Jp)^-1 (tau - C dq - m Jp^T (dJp dq)
    - g - Jp^T m (0, 0, -9.81)^T) with Jp, dJp the linear rows of J / dJ("EE", x=r).  effects, tau_ext and wrench stay
    optional.  Host arrays or DeviceArrays, never mixed."""
    if payload is None:
        return engine.forward_dynamics(arm_id, n, q, dq, u, ddq, dtype, device, stream, effects, tau_ext, wrench)
    a = engine._Args(dtype, device)
    B = q.shape[0]
    qp, dqp, up = a.inp(q, (B, n), "q"), a.inp(dq, (B, n), "dq"), a.inp(u, (B, n), "u")
    ep, wp = a.inp(tau_ext, (B, n), "tau_ext"), a.inp(wrench, (B, 6), "wrench")
    pp = a.inp(payload, (B, 4), "payload")
    op, oo = a.out(ddq, (B, n), "ddq")
    check(engine.lib().abrk_forward_dynamics_payload_batch(
        arm_id, a.code, None if effects is None else C.byref(effects), B, qp, dqp, up, ep, wp, pp, op, device,
        engine._sp(stream)))
    return oo


def plant_step(arm_id, n, params, q, dq, u, dtype=np.float64, device=0, stream=None, effects=None, tau_ext=None,
               wrench=None, payload=None):
    """engine.plant_step for rows that carry `payload` [B,4]: (q, dq) advanced in place.  Recorded into a plan, the
    kernel reads the payload array at every replay - rewriting it between two launches is a pick-up or a drop.  A host
    array with a negative or non-finite m, or a non-finite r, is refused naming the row; a DeviceArray is not looked at."""
    if payload is None:
        return engine.plant_step(arm_id, n, params, q, dq, u, dtype, device, stream, effects, tau_ext, wrench)
    a = engine._Args(dtype, device)
    B = q.shape[0]
    qp, dqp = a.inout(q, (B, n), "q"), a.inout(dq, (B, n), "dq")
    up = a.inp(u, (B, n), "u")
    ep, wp = a.inp(tau_ext, (B, n), "tau_ext"), a.inp(wrench, (B, 6), "wrench")
    pp = a.inp(payload, (B, 4), "payload")
    check(engine.lib().abrk_plant_step_payload_batch(
        arm_id, a.code, C.byref(params), None if effects is None else C.byref(effects), B, qp, dqp, up, ep, wp, pp,
        device, engine._sp(stream)))
