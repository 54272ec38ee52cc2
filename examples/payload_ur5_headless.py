"""A carried mass the controller does not know of, different on every arm: B UR5 arms follow planned paths on the device
with an empty gripper; half-way the payload array is rewritten - each arm now carries its own 0 - 3 kg, 5 cm beyond the
end effector - and the run goes on.  The payload is part of the PLANT (plant_payload.plant_step(payload=...): it changes M, C
and g of that arm), the OSC law keeps the robot_config's model, so its tracking error grows with the mass; the adaptive
signal (controllers.signals.DynamicsAdaptation), trained by the law's own training_signal, learns the torques that carry
it.  The tick

    { path_next; OSC.generate(training_signal=ts); [adapt.step(q, dq, ts, u_add=u);] plant step with payload; record }

is recorded once into one engine.Plan and replayed with launch_graph; the kernel reads the payload array at every replay,
so rewriting it between two launches is all it takes.  Prints the recorder's statistics of the two halves, with and
without the adaptive signal.

    python examples/payload_ur5_headless.py [--arms 4096] [--ticks 3000] [--neurons 1000]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout

import abr_control_amd as a
from abr_control_amd import _abi, engine, plant_payload
from abr_control_amd.arms import ur5
from abr_control_amd.controllers.path_planners import PathPlanner, position_profiles, velocity_profiles
from abr_control_amd.controllers.signals import DynamicsAdaptation

CHUNK = 500  # ticks per graph launch


def run(adaptive, B, ticks, n_neurons, dt=0.001):
    """-> (statistics of the first half: no payload, statistics of the second half: 0 - 3 kg per arm, the masses)"""
    rc = ur5.Config()
    n = rc.N_JOINTS
    rng = np.random.RandomState(0)
    q0 = rng.uniform(-1.0, 1.0, (B, n))
    start, target = rc.Tx("EE", q0), rc.Tx("EE", q0 + 0.2)
    empty = np.zeros((B, 4))
    carried = np.concatenate([rng.uniform(0.0, 3.0, (B, 1)), np.tile([0.0, 0.0, 0.05], (B, 1))], axis=1)

    stream = a.Stream(0)
    planner = PathPlanner(position_profiles.Linear(), velocity_profiles.Gaussian(dt=dt, acceleration=2), stream=stream)
    planner.generate_path(start, target, max_velocity=1.0, start_orientation=np.zeros((B, 3)),
                          target_orientation=np.zeros((B, 3)), to_host=False)
    path, n_timesteps = planner.device_path()
    q, dq, u, load = (a.DeviceArray.from_numpy(x) for x in (q0, np.zeros((B, n)), np.zeros((B, n)), empty))
    tgt, tgt_v = a.DeviceArray((B, 6)).zero_(stream), a.DeviceArray((B, 6)).zero_(stream)
    ts = a.DeviceArray((B, n)).zero_(stream)
    counter = a.DeviceArray((B,), np.int32).zero_(stream)
    law = _abi.make_osc_params(n, kp=200, use_C=True, use_g=True)
    plant = _abi.make_plant_params(dt, substeps=2)
    rec = a.LoopRecorder(rc, B, columns=("err",), tol=0.005, stream=stream)
    adapt = None
    if adaptive:
        r2 = np.random.RandomState(0)
        adapt = DynamicsAdaptation(
            n_input=2 * n, n_output=n, n_neurons=n_neurons, seed=0, pes_learning_rate=2e-4,
            intercepts=r2.uniform(-0.5, 0.3, n_neurons), means=np.zeros(2 * n), variances=np.full(2 * n, 2.0),
            neuron_type="lif_rate", stream=stream)
    with engine.Plan(device=0, stream=stream) as tick:
        engine.path_next(path, n_timesteps, counter, tgt, tgt_v, stream=stream)
        engine.osc_generate(rc.arm_id, n, law, q, dq, tgt, target_velocity=tgt_v, u=u, training_signal=ts, stream=stream)
        if adaptive:
            adapt.step(q, dq, ts, u_add=u)
        plant_payload.plant_step(rc.arm_id, n, plant, q, dq, u, stream=stream, payload=load)
        rec.record(q, dq, u, tgt)

    def replay(k):
        while k > 0:
            tick.launch_graph(min(k, CHUNK))
            k -= CHUNK

    half = ticks // 2
    replay(half)
    first = rec.stats()
    load.copy_from_numpy(carried, stream=stream)  # the grippers close: the next replay reads the new masses
    rec.reset()
    replay(ticks - half)
    second = rec.stats()
    assert np.isfinite(q.numpy(stream)).all()
    return first, second, carried[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=3000, help="ticks of 1 ms in all; the payload arrives half-way")
    ap.add_argument("--neurons", type=int, default=1000)
    args = ap.parse_args()
    print(f"{args.arms} UR5 arms, {args.ticks} ticks of 1 ms; from tick {args.ticks // 2} on every arm carries its own "
          f"0 - 3 kg, 5 cm beyond the end effector")
    for adaptive in (False, True):
        first, second, m = run(adaptive, args.arms, args.ticks, args.neurons)
        heavy = m > 2.0 if (m > 2.0).any() else m >= 0
        name = "with adaptation:   " if adaptive else "without adaptation:"
        print(f"{name} err_rms empty {first['err_rms'].mean() * 1e3:.3f} mm; carrying {second['err_rms'].mean() * 1e3:.3f} mm"
              f" (arms above 2 kg {second['err_rms'][heavy].mean() * 1e3:.3f} mm, worst arm "
              f"{second['err_rms'].max() * 1e3:.3f} mm); err_last {second['err_last'].mean() * 1e3:.3f} mm")


if __name__ == "__main__":
    main()
