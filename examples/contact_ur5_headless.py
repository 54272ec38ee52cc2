"""Touching a table, on the device: B UR5 arms, each above a table of its own height and stiffness, press down on it,
slide along it against friction and lift off again.  The table is part of the PLANT - the OSC law knows nothing of it and
simply follows its path, whose points lie below the table top while the arm is meant to press - and the contact kernel
(ContactSurfaces.apply, abrk_contact_step_batch) turns each arm's penetration into the joint torque the plant step reads
as tau_ext.  The tick

    { path_next; OSC.generate; contact; plant step }

is recorded into one engine.Plan per phase and replayed with launch_graph; the host only reads the force report at the
end of each phase.  The contact force is that of the state at the start of the tick (include/abrk.h): with k up to
2e4 N/m, dt = 1 ms and an effective mass of a few kg, k dt^2 / m_eff stays below 0.05.

    python examples/contact_ur5_headless.py [--arms 4096] [--settle 400]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout

import abr_control_amd as a
from abr_control_amd import _abi, engine
from abr_control_amd.arms import ur5
from abr_control_amd.controllers.path_planners import PathPlanner, position_profiles, velocity_profiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", type=int, default=4096)
    ap.add_argument("--settle", type=int, default=400, help="ticks of 1 ms a phase goes on after its longest path ends")
    args = ap.parse_args()
    B, dt = args.arms, 0.001
    rc = ur5.Config()
    n = rc.N_JOINTS
    rng = np.random.RandomState(0)
    q0 = np.asarray(rc.START_ANGLES, dtype=float) + rng.uniform(-0.3, 0.3, (B, n))
    p0 = rc.Tx("EE", q0)
    # every arm its own table: 2 - 6 cm below its end effector, 5e3 - 2e4 N/m, friction coefficient 0.2 - 0.6
    gap, k, mu = rng.uniform(0.02, 0.06, B), rng.uniform(5e3, 2e4, B), rng.uniform(0.2, 0.6, B)
    planes = np.zeros((B, 1, 8))
    planes[:, 0, 2] = 1.0
    planes[:, 0, 3] = p0[:, 2] - gap
    planes[:, 0, 4], planes[:, 0, 5], planes[:, 0, 6], planes[:, 0, 7] = k, 2.0 * np.sqrt(k), mu, 0.005
    # way points of the law: 12 cm below the table top (this law, kp = 200 without an integral term, stops several cm short
    # of a target it is held away from: how hard it presses is kp times that distance), 10 cm along it, 25 cm up
    down = p0 - np.stack([np.zeros(B), np.zeros(B), gap + 0.12], axis=1)
    along = down + np.array([0.10, 0.0, 0.0])
    up = along + np.array([0.0, 0.0, 0.37])

    stream = a.Stream(0)
    table = a.ContactSurfaces(rc, B, planes, vs=0.01, stream=stream)
    q, dq, u = (a.DeviceArray.from_numpy(x) for x in (q0, np.zeros((B, n)), np.zeros((B, n))))
    law = _abi.make_osc_params(n, kp=200, use_C=True, use_g=True)
    plant = _abi.make_plant_params(dt, substeps=1)
    print(f"{B} UR5 arms, tables 2 - 6 cm below them, k 5e3 - 2e4 N/m, mu 0.2 - 0.6; ticks of 1 ms")
    for name, start, target in (("press", p0, down), ("slide", down, along), ("lift", along, up)):
        planner = PathPlanner(position_profiles.Linear(), velocity_profiles.Gaussian(dt=dt, acceleration=2), stream=stream)
        planner.generate_path(start, target, max_velocity=0.5, start_orientation=np.zeros((B, 3)),
                              target_orientation=np.zeros((B, 3)), to_host=False)
        path, n_timesteps = planner.device_path()
        ticks = int(planner.n_timesteps.max()) + args.settle
        tgt, tgt_v = a.DeviceArray((B, 6)).zero_(stream), a.DeviceArray((B, 6)).zero_(stream)
        counter = a.DeviceArray((B,), np.int32).zero_(stream)
        with engine.Plan(device=0, stream=stream) as tick:
            engine.path_next(path, n_timesteps, counter, tgt, tgt_v, stream=stream)
            engine.osc_generate(rc.arm_id, n, law, q, dq, tgt, target_velocity=tgt_v, u=u, stream=stream)
            tau_c = table.apply(q, dq)
            engine.plant_step(rc.arm_id, n, plant, q, dq, u, stream=stream, tau_ext=tau_c)
        tick.launch_graph(ticks)
        r = table.report()
        touching = r["n_contacts"] > 0
        fz, ft = r["force"][:, 2], np.linalg.norm(r["force"][:, :2], axis=1)
        line = f"{name:5s} ({ticks} ticks): {int(touching.sum())} of {B} arms touch their table"
        if touching.any():
            line += (f"; normal force {fz[touching].mean():.2f} N (max {fz.max():.2f}), depth "
                     f"{r['depth'][touching].mean() * 1e3:.2f} mm, friction / normal "
                     f"{(ft[touching] / np.maximum(fz[touching], 1e-9)).mean():.2f}")
        else:
            line += f"; clearance {-r['depth'].mean() * 1e3:.1f} mm"
        print(line)
        assert np.isfinite(q.numpy(stream)).all()
    assert not touching.any(), "the arms did not lift off"


if __name__ == "__main__":
    main()
