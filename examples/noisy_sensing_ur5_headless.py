"""Sensing that is not exact, for B UR5 arms entirely on the device: the loop of closed_loop_ur5_headless.py, in which the
law no longer reads the plant's own q and dq.  A JointSensor stands between them: 14-bit encoders (2 pi / 2^14 rad per
count), two ticks of latency, and a velocity that is the low-passed difference of consecutive encoder readings.  The tick

    { sensor.measure(q, dq) -> q_meas, dq_meas; OSC.generate on q_meas, dq_meas; plant step; record }

is recorded once into one engine.Plan and replayed with launch_graph: the encoder's delay ring, the differencer's state
and the tick counters live in device memory and advance at every replay.  Run with and without the sensor and print the
tracking error (err_rms over the last ticks).

    python examples/noisy_sensing_ur5_headless.py [B] [ticks]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout

import abr_control_amd as a
from abr_control_amd import _abi, engine
from abr_control_amd.arms import ur5

ENCODER_BITS, LATENCY_TICKS, TAU_VELOCITY = 14, 2, 0.005


def run(sensed, B, ticks, last=100, dt=0.001):
    """-> the recorder's statistics over the last `last` of `ticks` ticks"""
    rc = ur5.Config()
    n = rc.N_JOINTS
    rng = np.random.RandomState(0)
    q0 = rng.uniform(-1.0, 1.0, (B, n))
    target = np.zeros((B, 6))
    target[:, :3] = rc.Tx("EE", q0 + 0.1)  # a reachable point per arm

    stream = a.Stream(0)
    q, dq, u, tgt = (a.DeviceArray.from_numpy(x) for x in (q0, np.zeros((B, n)), np.zeros((B, n)), target))
    law = _abi.make_osc_params(n, kp=100, use_C=True, use_g=True)
    plant = _abi.make_plant_params(dt, substeps=2)
    rec = a.LoopRecorder(rc, B, columns=("err",), tol=0.005, stream=stream)
    sensor = a.JointSensor(rc, B, resolution=2 * np.pi / 2 ** ENCODER_BITS, delay=LATENCY_TICKS, velocity="difference",
                           tau_velocity=TAU_VELOCITY, dt=dt, stream=stream) if sensed else None
    with engine.Plan(device=0, stream=stream) as tick:
        q_meas, dq_meas = sensor.measure(q, dq) if sensed else (q, dq)
        engine.osc_generate(rc.arm_id, n, law, q_meas, dq_meas, tgt, u=u, stream=stream)
        engine.plant_step(rc.arm_id, n, plant, q, dq, u, stream=stream)
        rec.record(q, dq, u, tgt)  # the error of the plant's true state
    tick.launch_graph(ticks - last)
    rec.reset()
    tick.launch_graph(last)
    stats = rec.stats()
    assert np.isfinite(q.numpy(stream)).all()
    return stats


def main(B=64, ticks=400):
    print(f"{B} UR5 arms, {ticks} ticks of 1 ms; sensor: {ENCODER_BITS}-bit encoders, {LATENCY_TICKS} ticks of latency, "
          f"velocity from differenced readings (tau {TAU_VELOCITY * 1e3:g} ms)")
    exact = run(False, B, ticks)["err_rms"]
    sensed = run(True, B, ticks)["err_rms"]
    print(f"exact state:  err_rms over the last 100 ticks {exact.mean() * 1e3:.3f} mm (worst arm {exact.max() * 1e3:.3f} mm)")
    print(f"through the sensor: err_rms over the last 100 ticks {sensed.mean() * 1e3:.3f} mm (worst arm "
          f"{sensed.max() * 1e3:.3f} mm)")


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:3]))
