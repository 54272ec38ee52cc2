"""Closed loop for B UR5 arms entirely on the device: the tick is OSC.generate (x,y,z, use_C, use_g) followed by the
rigid-body plant step, RECORDED once into one engine.Plan and then replayed as a hipGraph - the host neither computes
nor copies anything between ticks.

    python examples/closed_loop_ur5_headless.py [B] [ticks]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout

import abr_control_amd as a
from abr_control_amd import _abi, engine
from abr_control_amd.arms import ur5


def main(B=256, ticks=1000, dt=0.001):
    rc = ur5.Config()
    n = rc.N_JOINTS
    rng = np.random.RandomState(0)
    q0 = rng.uniform(-1.0, 1.0, (B, n))
    target = np.zeros((B, 6))
    target[:, :3] = rc.Tx("EE", q0 + 0.2)  # a reachable point per arm

    def error(q):
        return float(np.mean(np.linalg.norm(rc.Tx("EE", q) - target[:, :3], axis=1)))

    stream = a.Stream(0)
    q, dq, tgt, u = (a.DeviceArray.from_numpy(x) for x in (q0, np.zeros((B, n)), target, np.zeros((B, n))))
    law = _abi.make_osc_params(n, kp=200, use_C=True, use_g=True)
    plant = _abi.make_plant_params(dt, substeps=1, gravity=True)
    with engine.Plan(device=0, stream=stream) as tick:
        engine.osc_generate(rc.arm_id, n, law, q, dq, tgt, u=u, stream=stream)
        engine.plant_step(rc.arm_id, n, plant, q, dq, u, stream=stream)
    before = error(q0)
    tick.launch_graph(ticks)
    stream.sync()
    after = error(q.numpy())
    print(f"{B} UR5 arms, {ticks} ticks of {dt * 1e3:g} ms: mean end-effector error {before:.4f} m -> {after:.4f} m")
    assert after < before, "the loop did not close"


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:3]))
