#!/usr/bin/env python3
"""Timing of the rigid-body plant step on UR5 fp64 (development aid; bench.py does not cover the plant).

HIP events on the launch stream, 12 warm-up and 30 timed launches per figure; prints ONE JSON line:
  plant_us[rows][substeps]      plant_step alone at 4096 and 8 M rows, substeps 1 and 100
  osc_cfg4_us[rows]             the x,y,z + use_C + use_g OSC kernel alone, same process
  tick_graph_us                 the recorded {OSC cfg4; plant step} tick at 4096 rows, launch_graph(2000), per tick

    python tools/plant_timing.py [--rows-large 8388608]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP, TIMED = 12, 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-large", type=int, default=8 << 20)
    args = ap.parse_args()
    import abr_control_amd as a
    from abr_control_amd import _abi, engine
    from abr_control_amd.arms import ur5

    rc = ur5.Config()
    n = 6
    s = a.Stream(0)
    law = _abi.make_osc_params(n, kp=200, use_C=True, use_g=True)

    def timed(fn, launches=TIMED, per=1):
        for _ in range(WARMUP):
            fn()
        s.sync()
        e0, e1 = a.Event(0), a.Event(0)
        ts = []
        for _ in range(launches):
            e0.record(s)
            fn()
            e1.record(s)
            s.sync()
            ts.append(e1.elapsed_ms_since(e0) * 1e3 / per)
        return {"median_us": float(np.median(ts)), "min_us": float(np.min(ts)), "max_us": float(np.max(ts))}

    res = {"arm": "ur5", "dtype": "float64", "device": a.device_name(0), "warmup": WARMUP, "timed": TIMED,
           "plant_us": {}, "osc_cfg4_us": {}}
    rng = np.random.RandomState(0)
    for B in (4096, args.rows_large):
        q0 = rng.uniform(-np.pi, np.pi, (B, n))
        q, dq, u, t = (a.DeviceArray.from_numpy(x) for x in (q0, np.zeros((B, n)), rng.uniform(-20, 20, (B, n)),
                                                             rng.uniform(-1, 1, (B, 6))))
        uo = a.DeviceArray.from_numpy(np.zeros((B, n)))
        res["plant_us"][str(B)] = {}
        for sub in (1, 100):
            # dt scales with the substeps: every substep is 10 us of simulated time and the state stays bounded
            p = _abi.make_plant_params(1e-5 * sub, substeps=sub)
            res["plant_us"][str(B)][str(sub)] = timed(lambda: engine.plant_step(rc.arm_id, n, p, q, dq, u, stream=s))
        res["osc_cfg4_us"][str(B)] = timed(lambda: engine.osc_generate(rc.arm_id, n, law, q, dq, t, u=uo, stream=s))
        if B == 4096:
            p1 = _abi.make_plant_params(1e-3)
            with engine.Plan(device=0, stream=s) as tick:
                engine.osc_generate(rc.arm_id, n, law, q, dq, t, u=uo, stream=s)
                engine.plant_step(rc.arm_id, n, p1, q, dq, uo, stream=s)
            res["tick_graph_us"] = timed(lambda: tick.launch_graph(2000), launches=5, per=2000)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
