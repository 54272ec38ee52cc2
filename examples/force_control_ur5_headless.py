"""Pressing on a table with a commanded force, on the device: B UR5 arms approach a floor 2 cm below them, touch it, build
up the force each was told to press with and slide 6 cm along it - Khatib's unified motion/force law
(ForceController.generate, abrk_force_control_batch) in place of the motion law of examples/contact_ur5_headless.py, which
can only press with kp times the distance its target lies below the surface.  The tick

    { force law (reads the contact report of the previous tick); contact; plant step; recorder }

is recorded into one engine.Plan and replayed with launch_graph; the host reads the force report and the recorder's
statistics between phases.  The floor is part of the PLANT; the law sees it only through the reported force: while that
is below f_touch it approaches along -n at v_app, above it it runs a PI loop on the force along n and the motion law in
the tangent plane.  Rows cycle through f_des in {5, 10, 20} N, k in {5e3, 2e4} N/m and mu in {0, 0.4}; with mu > 0 the
tangential target is reached up to what friction holds back (no integral term in the tangent plane).  Halfway, every
row's desired force is raised by half through set_command: the recorded plan reads the command at replay.

Gravity is off in the law and in the plant: both subtract the same robot_config.g, and switched on together they lift the
tip off its target.  The recorder's target carries, in z, the height at which the tip rests when it
presses with f_des (d + rho - f_des / k) - the law itself ignores the target along n - so that its error statistics are
the distance to where the tip should end up.

    python examples/force_control_ur5_headless.py [--arms 4096] [--ticks 1500]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout

import abr_control_amd as a
from abr_control_amd import _abi, engine
from abr_control_amd.arms import ur5

GAINS = dict(kp=100.0, kv=20.0, kf=0.5, ki=20.0, i_max=50.0, kvf=20.0, f_touch=0.5, v_app=0.05, kv_null=10.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=1500, help="ticks of 1 ms per phase")
    args = ap.parse_args()
    B, dt = args.arms, 0.001
    rc = ur5.Config()
    n = rc.N_JOINTS
    q0 = np.tile([0.3, -1.2, 1.6, -0.5, 1.2, 0.2], (B, 1))
    p0 = rc.Tx("EE", q0)
    b = np.arange(B)
    f_des = np.array([5.0, 10.0, 20.0])[b % 3]
    k = np.array([5e3, 2e4])[(b // 3) % 2]
    mu = np.array([0.0, 0.4])[(b // 6) % 2]
    rho = 0.005
    planes = np.zeros((B, 1, 8))
    planes[:, 0, 2] = 1.0
    planes[:, 0, 3] = p0[:, 2] - 0.02
    planes[:, 0, 4], planes[:, 0, 5], planes[:, 0, 6], planes[:, 0, 7] = k, 200.0, mu, rho
    target = np.zeros((B, 6))
    target[:, :3] = p0 + np.array([0.05, 0.03, 0.0])

    def resting(f):
        t = target.copy()
        t[:, 2] = planes[:, 0, 3] + rho - f / k
        return t

    stream = a.Stream(0)
    table = a.ContactSurfaces(rc, B, planes, stream=stream)
    press = a.ForceController(rc, B, (0, 0, 1), f_des, dt=dt, stream=stream, use_g=False, **GAINS)
    rec = a.LoopRecorder(rc, B, tol=1e-4, stream=stream)
    q, dq, tgt = (a.DeviceArray.from_numpy(x) for x in (q0, np.zeros((B, n)), resting(f_des)))
    report = table.device_arrays()["report"].zero_(stream)
    plant = _abi.make_plant_params(dt, substeps=1, gravity=False)
    with engine.Plan(device=0, stream=stream) as tick:
        u = press.generate(q, dq, tgt, report)
        tau_c = table.apply(q, dq)
        engine.plant_step(rc.arm_id, n, plant, q, dq, u, stream=stream, tau_ext=tau_c)
        rec.record(q, dq, u, tgt)
    print(f"{B} UR5 arms, a floor 2 cm below them, k 5e3 / 2e4 N/m, mu 0 / 0.4, f_des 5 / 10 / 20 N; ticks of 1 ms")
    for name, want in (("press", f_des), ("press 1.5 x harder", 1.5 * f_des)):
        if want is not f_des:
            press.set_command(f_des=want)
            tgt.copy_from_numpy(resting(want), stream)
            rec.reset()
        tick.launch_graph(args.ticks)
        r, st = table.report(), rec.stats()
        dev = np.abs(r["force"][:, 2] - want) / want
        free = mu == 0
        print(f"{name} ({args.ticks} ticks): {int((r['n_contacts'] > 0).sum())} of {B} arms touch; |F_z - f_des| / f_des "
              f"max {dev.max():.1e}; distance to the resting point, mu = 0 rows: last {st['err_last'][free].max():.1e} m, "
              f"rms {st['err_rms'][free].max():.1e} m; mu = 0.4 rows: last {st['err_last'][~free].max():.1e} m; within "
              f"0.1 mm since tick {int(np.where(free, st['settle_tick'], 0).max())} at the latest (mu = 0)")
        assert np.isfinite(q.numpy(stream)).all()
        assert dev.max() <= 1e-2, "the arms do not press with the commanded force"


if __name__ == "__main__":
    main()
