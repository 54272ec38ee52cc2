"""Disturbance rejection for B UR5 arms entirely on the device.  The plant is NOT the controller's model: its joints have
viscous and Coulomb friction the controller does not know of, its motors saturate, its joints have hard limits, and half
way through the run a force pushes on every end effector.  The tick { OSC.generate; plant step with effects;
LoopRecorder.record } is recorded once into one engine.Plan and replayed with launch_graph; the wrench is switched on
between two launch_graph calls by writing the device array the recorded plant step reads - the plan itself is not touched.
Run twice, with ki = 0 and with an integral term (the reference's law sums the error per tick, so ki is small), and print the tracking error (err_rms over the phase) before and under
the load.

    python examples/disturbance_rejection_ur5_headless.py [B] [ticks per phase]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout

import abr_control_amd as a
from abr_control_amd import _abi, engine
from abr_control_amd.arms import ur5


def run(ki, B, ticks, dt=0.001, force=(0.0, 0.0, -15.0)):
    rc = ur5.Config()
    n = rc.N_JOINTS
    rng = np.random.RandomState(0)
    q0 = rng.uniform(-1.0, 1.0, (B, n))
    target = np.zeros((B, 6))
    target[:, :3] = rc.Tx("EE", q0 + 0.1)  # a reachable point per arm

    stream = a.Stream(0)
    q, dq, u, tgt = (a.DeviceArray.from_numpy(x) for x in (q0, np.zeros((B, n)), np.zeros((B, n)), target))
    ierr = a.DeviceArray((B, 6)).zero_(stream)
    wrench = a.DeviceArray((B, 6)).zero_(stream)  # [fx fy fz mx my mz] in the world frame, at the end effector
    law = _abi.make_osc_params(n, kp=200, ki=ki, use_C=True, use_g=True)
    plant = _abi.make_plant_params(dt, substeps=2)
    effects = _abi.make_plant_effects(n, damping=0.5, coulomb=0.3, coulomb_vs=0.01, tau_max=150.0, q_min=-2 * np.pi,
                                      q_max=2 * np.pi, restitution=0.0)
    rec = a.LoopRecorder(rc, B, columns=("err",), tol=0.005, stream=stream)
    with engine.Plan(device=0, stream=stream) as tick:
        engine.osc_generate(rc.arm_id, n, law, q, dq, tgt, integrated_error=ierr if ki else None, u=u, stream=stream)
        engine.plant_step(rc.arm_id, n, plant, q, dq, u, stream=stream, effects=effects, wrench=wrench)
        rec.record(q, dq, u, tgt)

    tick.launch_graph(ticks)  # reach the target: friction and saturation only
    rec.reset()
    tick.launch_graph(ticks)  # hold it
    before = rec.stats()
    w = np.zeros((B, 6))
    w[:, :3] = force
    wrench.copy_from_numpy(w, stream=stream)  # the load comes on: the recorded plant step reads this array every tick
    rec.reset()
    tick.launch_graph(ticks)
    under = rec.stats()
    assert np.isfinite(q.numpy(stream)).all()
    return before, under


def main(B=4096, ticks=1500):
    print(f"{B} UR5 arms, {ticks} ticks of 1 ms per phase; load: 15 N downwards on every end effector")
    for ki in (0.0, 0.1):
        before, under = run(ki, B, ticks)
        print(f"ki = {ki:g}: err_rms holding the target {before['err_rms'].mean() * 1e3:.3f} mm -> under the load "
              f"{under['err_rms'].mean() * 1e3:.3f} mm (error at the end {under['err_last'].mean() * 1e3:.3f} mm)")


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:3]))
