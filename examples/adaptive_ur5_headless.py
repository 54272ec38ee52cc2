"""Dynamics adaptation for B UR5 arms entirely on the device: the loop of disturbance_rejection_ur5_headless.py - a plant
with friction, saturation and joint limits the controller does not know of, and a force that pushes on every end effector
from the first tick on - with the adaptive signal as its fourth kernel.  The OSC law cannot learn the load, so its
steady-state error stays; a population of LIF neurons per arm (controllers.signals.DynamicsAdaptation), fed q and dq and
trained by the law's own training_signal, learns the torques that cancel it and adds them to u.  The tick

    { OSC.generate(training_signal=ts); adapt.step(q, dq, ts, u_add=u); plant step with effects and wrench; record }

is recorded once into one engine.Plan and replayed with launch_graph; the neurons' state and weights live in device
memory and advance at every replay.  Run with and without the adaptive signal and print the tracking error (err_rms
over the last ticks).

    python examples/adaptive_ur5_headless.py [B] [ticks]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout

import abr_control_amd as a
from abr_control_amd import _abi, engine
from abr_control_amd.arms import ur5
from abr_control_amd.controllers.signals import DynamicsAdaptation

CHUNK = 500  # ticks per graph launch


def make_adapt(n, n_neurons, pes_learning_rate, neuron_type, stream, seed=0):
    """one population per arm over (q, dq) scaled into about +-1; the intercepts are given, so scipy is not needed"""
    rng = np.random.RandomState(seed)
    return DynamicsAdaptation(
        n_input=2 * n, n_output=n, n_neurons=n_neurons, seed=seed, pes_learning_rate=pes_learning_rate,
        intercepts=rng.uniform(-0.5, 0.3, n_neurons), means=np.zeros(2 * n),
        variances=np.concatenate([np.full(n, 2.0), np.full(n, 2.0)]), neuron_type=neuron_type, stream=stream)


def run(adaptive, B, ticks, last=500, pes_learning_rate=2e-4, n_neurons=1000, neuron_type="lif_rate", dt=0.001,
        force=(0.0, 0.0, -15.0)):
    """-> the recorder's statistics over the last `last` of `ticks` ticks"""
    rc = ur5.Config()
    n = rc.N_JOINTS
    rng = np.random.RandomState(0)
    q0 = rng.uniform(-1.0, 1.0, (B, n))
    target = np.zeros((B, 6))
    target[:, :3] = rc.Tx("EE", q0 + 0.1)  # a reachable point per arm
    w = np.zeros((B, 6))
    w[:, :3] = force  # [fx fy fz mx my mz] in the world frame, at the end effector: on from the first tick

    stream = a.Stream(0)
    q, dq, u, tgt, wrench = (a.DeviceArray.from_numpy(x) for x in (q0, np.zeros((B, n)), np.zeros((B, n)), target, w))
    ts = a.DeviceArray((B, n)).zero_(stream)
    law = _abi.make_osc_params(n, kp=200, use_C=True, use_g=True)
    plant = _abi.make_plant_params(dt, substeps=2)
    effects = _abi.make_plant_effects(n, damping=0.5, coulomb=0.3, coulomb_vs=0.01, tau_max=150.0, q_min=-2 * np.pi,
                                      q_max=2 * np.pi, restitution=0.0)
    rec = a.LoopRecorder(rc, B, columns=("err",), tol=0.005, stream=stream)
    adapt = make_adapt(n, n_neurons, pes_learning_rate, neuron_type, stream) if adaptive else None
    with engine.Plan(device=0, stream=stream) as tick:
        engine.osc_generate(rc.arm_id, n, law, q, dq, tgt, u=u, training_signal=ts, stream=stream)
        if adaptive:
            adapt.step(q, dq, ts, u_add=u)
        engine.plant_step(rc.arm_id, n, plant, q, dq, u, stream=stream, effects=effects, wrench=wrench)
        rec.record(q, dq, u, tgt)

    def replay(k):
        while k > 0:
            tick.launch_graph(min(k, CHUNK))
            k -= CHUNK

    replay(ticks - last)
    rec.reset()
    replay(last)
    stats = rec.stats()
    assert np.isfinite(q.numpy(stream)).all()
    return stats


def main(B=256, ticks=3000):
    print(f"{B} UR5 arms, {ticks} ticks of 1 ms; load: 15 N downwards on every end effector from the first tick on")
    plain = run(False, B, ticks)["err_rms"]
    adaptive = run(True, B, ticks)["err_rms"]
    print(f"without adaptation: err_rms over the last 500 ticks {plain.mean() * 1e3:.3f} mm (worst arm {plain.max() * 1e3:.3f} mm)")
    print(f"with adaptation:    err_rms over the last 500 ticks {adaptive.mean() * 1e3:.3f} mm (worst arm "
          f"{adaptive.max() * 1e3:.3f} mm); smallest ratio over the arms {np.min(plain / adaptive):.1f}")


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:3]))
