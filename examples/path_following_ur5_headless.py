"""Path following for B UR5 arms entirely on the device: every arm gets its own start (where its end effector is) and
target, PathPlanner plans all B paths in one generate_path call - Gaussian velocity profile, orientation by SLERP -
and the tick { path_next; OSC.generate with target_velocity; plant step; LoopRecorder.record } is RECORDED once into one
engine.Plan and replayed as ONE hipGraph launch: each tick reads its own path point on the device and leaves its tracking
error in the recorder's per-arm statistics and decimated history - the host neither computes nor copies until the end.

    python examples/path_following_ur5_headless.py [B] [settle ticks]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout

import abr_control_amd as a
from abr_control_amd import _abi, engine
from abr_control_amd.arms import ur5
from abr_control_amd.controllers.path_planners import PathPlanner, position_profiles, velocity_profiles


def main(B=4096, settle=500, dt=0.001, tol=0.02):
    rc = ur5.Config()
    n = rc.N_JOINTS
    rng = np.random.RandomState(0)
    q0 = rng.uniform(-1.0, 1.0, (B, n))
    start = rc.Tx("EE", q0)
    target = rc.Tx("EE", q0 + 0.2)  # a reachable point per arm

    stream = a.Stream(0)
    planner = PathPlanner(position_profiles.Linear(), velocity_profiles.Gaussian(dt=dt, acceleration=2), stream=stream)
    planner.generate_path(start, target, max_velocity=1.0, start_orientation=np.zeros((B, 3)),
                          target_orientation=np.zeros((B, 3)), to_host=False)
    path, n_timesteps = planner.device_path()
    steps = planner.n_timesteps
    print(f"{B} paths planned on the device: {steps.min()}..{steps.max()} steps of {dt * 1e3:g} ms")

    q, dq, u = (a.DeviceArray.from_numpy(x) for x in (q0, np.zeros((B, n)), np.zeros((B, n))))
    # (zero fills on the stream that consumes them: it does not order against the NULL stream)
    tgt, tgt_v = a.DeviceArray((B, 6)).zero_(stream), a.DeviceArray((B, 6)).zero_(stream)
    counter = a.DeviceArray((B,), np.int32).zero_(stream)
    law = _abi.make_osc_params(n, kp=200, use_C=True, use_g=True)
    plant = _abi.make_plant_params(dt, substeps=1, gravity=True)
    ticks = int(steps.max()) + settle  # to the end of the longest path, then `settle` ticks of the last point
    every = 50
    rec = a.LoopRecorder(rc, B, capacity=-(-ticks // every), every=every, columns=("xyz", "err"), tol=tol, stream=stream)
    with engine.Plan(device=0, stream=stream) as tick:
        engine.path_next(path, n_timesteps, counter, tgt, tgt_v, stream=stream)
        engine.osc_generate(rc.arm_id, n, law, q, dq, tgt, target_velocity=tgt_v, u=u, stream=stream)
        engine.plant_step(rc.arm_id, n, plant, q, dq, u, stream=stream)
        rec.record(q, dq, u, tgt)

    tick.launch_graph(ticks)  # the whole run: one graph launch, no host round trip
    st, err = rec.stats(), rec.history()["err"][..., 0]
    half = int(np.median(steps)) // 2 // every  # half way along the median path: how far behind its path point is each arm?
    before, after = np.linalg.norm(start - target, axis=1).mean(), st["err_last"].mean()
    settled = st["settle_tick"] >= 0
    print(f"tick {half * every}: mean distance of the end effector to its path point {err[half].mean():.4f} m "
          f"(max {err[half].max():.4f}); over the run: rms {st['err_rms'].mean():.4f} m, worst {st['err_max'].max():.4f} m")
    print(f"tick {ticks}: mean distance to the target {before:.4f} m -> {after:.4f} m; {int(settled.sum())} of {B} arms within "
          f"{tol * 1e3:g} mm, since tick {int(np.median(st['settle_tick'][settled])) if settled.any() else -1} (median)")
    assert (st["ticks"] == ticks).all() and np.isfinite(q.numpy(stream)).all() and after < before, \
        "the arms did not follow their paths"


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:3]))
