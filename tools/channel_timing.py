#!/usr/bin/env python3
"""Timing of the measurement channel (development aid; bench.py does not cover it; numbers: profiles/sensing.md).

HIP events on the launch stream, 3 warm-up rounds, the median of 10 timed ones; prints ONE JSON line:
  loop_us[dtype]          { OSC; plant step } at 4096 UR5 rows inside a recorded plan, launch_graph(1000), per tick:
                          "plain", and "sensed" = the same plan with one JointSensor.measure (14-bit encoders, noise, two
                          ticks of latency, measured velocity: width 12) in front of the law and one SignalChannel.apply (one
                          tick of latency, width 6) behind it; "added_us" is the difference of the medians
  direct_us[dtype][kind]  the stand-alone tick at 1 M rows x 12 columns (in0 = in1 = [B,6]), delay 2, 20 launches back to
                          back, per tick: "quantised" (no sigma: the instantiation without the generator) and "noisy"
                          (sigma on every column); each with `hbm_fraction`: the algorithmic bytes - in, out, the ring
                          slot written and the ring slot read, the counter read and written - over the time, as a
                          fraction of the 8 TB/s HBM peak.

    python tools/channel_timing.py [--rows-graph 4096] [--rows-direct 1048576]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP, TIMED = 3, 10
W = 12
HBM_PEAK = 8e12
ENCODER = 2 * np.pi / 2 ** 14


def row_bytes(dtype):
    return 4 * W * np.dtype(dtype).itemsize + 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-graph", type=int, default=4096)
    ap.add_argument("--rows-direct", type=int, default=1 << 20)
    ap.add_argument("--graph-ticks", type=int, default=1000)
    args = ap.parse_args()
    import abr_control_amd as a
    from abr_control_amd import _abi, engine
    from abr_control_amd.arms import ur5

    s = a.Stream(0)
    e0, e1 = a.Event(0), a.Event(0)

    def timed(fn, per):
        for _ in range(WARMUP):
            fn()
        s.sync()
        ts = []
        for _ in range(TIMED):
            e0.record(s)
            fn()
            e1.record(s)
            s.sync()
            ts.append(e1.elapsed_ms_since(e0) * 1e3 / per)
        return {"median_us": float(np.median(ts)), "min_us": float(np.min(ts)), "max_us": float(np.max(ts))}

    rng = np.random.RandomState(0)
    res = {"device": a.device_name(0), "columns": W, "warmup": WARMUP, "timed": TIMED, "rows_graph": args.rows_graph,
           "rows_direct": args.rows_direct, "graph_ticks": args.graph_ticks, "loop_us": {}, "direct_us": {}}
    for dtype in (np.float64, np.float32):
        name = np.dtype(dtype).name
        rc = ur5.Config(dtype=dtype)
        n, B = rc.N_JOINTS, args.rows_graph
        q0 = rng.uniform(-1.0, 1.0, (B, n))
        target = np.zeros((B, 6))
        target[:, :3] = rc.Tx("EE", q0 + 0.1)
        law = _abi.make_osc_params(n, kp=100, use_C=True, use_g=True)
        plant = _abi.make_plant_params(1e-3, substeps=1)
        leg = {}
        for kind in ("plain", "sensed"):
            dev = lambda x: a.DeviceArray.from_numpy(np.ascontiguousarray(x, dtype=dtype))
            q, dq, u, tgt = dev(q0), dev(np.zeros((B, n))), dev(np.zeros((B, n))), dev(target)
            sensor = a.JointSensor(rc, B, resolution=ENCODER, noise_std=1e-4, noise_std_velocity=1e-3, delay=2, seed=1,
                                   stream=s)
            actuator = a.SignalChannel(n, B, delay=1, dtype=dtype, stream=s)
            with engine.Plan(device=0, stream=s) as tick:
                qm, dqm = sensor.measure(q, dq) if kind == "sensed" else (q, dq)
                engine.osc_generate(rc.arm_id, n, law, qm, dqm, tgt, u=u, dtype=dtype, stream=s)
                ua = actuator.apply(u) if kind == "sensed" else u
                engine.plant_step(rc.arm_id, n, plant, q, dq, ua, dtype=dtype, stream=s)
            leg[kind] = timed(lambda: tick.launch_graph(args.graph_ticks), per=args.graph_ticks)
            leg[kind]["finite"] = bool(np.isfinite(q.numpy(s)).all())
            tick.close()
        leg["added_us"] = leg["sensed"]["median_us"] - leg["plain"]["median_us"]
        res["loop_us"][name] = leg

        B = args.rows_direct
        x0, x1 = a.DeviceArray((B, W // 2), dtype).zero_(s), a.DeviceArray((B, W // 2), dtype).zero_(s)
        for kind, sigma in (("quantised", 0.0), ("noisy", 1e-3)):
            ch = a.SignalChannel(W, B, noise_std=sigma, resolution=ENCODER, delay=2, seed=1, dtype=dtype, stream=s)

            def burst():
                for _ in range(20):
                    ch.apply(x0, x1)
            r = timed(burst, per=20)
            r["bytes_per_row"] = row_bytes(dtype)
            r["hbm_fraction"] = B * r["bytes_per_row"] / (r["median_us"] * 1e-6) / HBM_PEAK
            res["direct_us"].setdefault(name, {})[kind] = r
            for arr in ch.device_state().values():
                arr.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
