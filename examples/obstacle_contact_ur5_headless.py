"""Hitting what the loop avoids, on the device: B UR5 arms reach for a target that lies behind a sphere.  The sphere is
part of the PLANT (Obstacles.apply, abrk_link_contact_step_batch: every link segment a capsule of 4 cm that the sphere
pushes back on), and it is also the obstacle of an AvoidObstacles controller - Obstacles.from_controller takes the
controller's own list.  The tick

    { OSC.generate; [AvoidObstacles.generate, added to u]; link contact; plant step }

is recorded into one engine.Plan and replayed with launch_graph, once with the avoidance term and once without; the
host reads the contact report between chunks of ticks.  Printed per run: the share of arms that touched the sphere, the
peak contact force and the smallest clearance between a capsule and the sphere (negative: penetration).

    python examples/obstacle_contact_ur5_headless.py [--arms 4096] [--ticks 1500]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout

import abr_control_amd as a
from abr_control_amd import _abi, engine
from abr_control_amd.arms import ur5
from abr_control_amd.controllers import AvoidObstacles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=1500, help="ticks of 1 ms per run")
    ap.add_argument("--chunk", type=int, default=25, help="ticks between two looks at the report")
    args = ap.parse_args()
    B, dt = args.arms, 0.001
    rc = ur5.Config()
    n = rc.N_JOINTS
    rng = np.random.RandomState(0)
    q0 = np.asarray(rc.START_ANGLES, dtype=float) + rng.uniform(-0.2, 0.2, (B, n))
    p_nom = np.asarray(rc.Tx("EE", np.asarray(rc.START_ANGLES, dtype=float)[None]))[0]
    reach = np.array([0.25, 0.25, -0.15])
    target = np.zeros((B, 6))
    target[:, :3] = p_nom + reach  # the same point for every arm, straight through the sphere
    sphere = [*(p_nom + 0.5 * reach), 0.06]
    avoid = AvoidObstacles(rc, obstacles=[sphere], threshold=0.2, gain=1, maximum=500)  # the reference's eta = 0.02
    stream = a.Stream(0)
    world = a.Obstacles.from_controller(avoid, B, k=2e4, c=2.0 * np.sqrt(2e4), mu=0.3, link_radius=0.04, stream=stream)
    law = _abi.make_osc_params(n, kp=100, use_C=True, use_g=True)
    plant = _abi.make_plant_params(dt, substeps=1)
    tgt = a.DeviceArray.from_numpy(target)
    print(f"{B} UR5 arms, a sphere of 6 cm half way to a target {np.linalg.norm(reach):.2f} m off, capsules of 4 cm, "
          f"k 2e4 N/m; {args.ticks} ticks of 1 ms")
    for name, avoiding in (("with AvoidObstacles", True), ("without", False)):
        q, dq, u = (a.DeviceArray.from_numpy(x) for x in (q0, np.zeros((B, n)), np.zeros((B, n))))
        with engine.Plan(device=0, stream=stream) as tick:
            engine.osc_generate(rc.arm_id, n, law, q, dq, tgt, u=u, stream=stream)
            if avoiding:
                engine.avoid_obstacles_generate(rc.arm_id, n, avoid._params(), q, u=u, accumulate=True, stream=stream)
            tau_c = world.apply(q, dq)
            engine.plant_step(rc.arm_id, n, plant, q, dq, u, stream=stream, tau_ext=tau_c)
        touched, peak, clearance = np.zeros(B, bool), 0.0, np.inf
        for _ in range(args.ticks // args.chunk):
            tick.launch_graph(args.chunk)
            r = world.report()
            touched |= r["n_contacts"] > 0
            peak = max(peak, float(np.linalg.norm(r["force"], axis=1).max()))
            clearance = min(clearance, float(-r["depth"].max()))
        err = np.linalg.norm(np.asarray(rc.Tx("EE", q.numpy(stream))) - target[:, :3], axis=1)
        print(f"{name:20s}: {100.0 * touched.mean():5.1f} % of the arms touched, peak force {peak:7.2f} N, smallest "
              f"clearance {clearance * 1e3:7.2f} mm; distance to the target at the end {err.mean() * 1e3:.1f} mm (mean)")
        assert np.isfinite(q.numpy(stream)).all()


if __name__ == "__main__":
    main()
