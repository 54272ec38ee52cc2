#!/usr/bin/env python3
"""Timing of the batched path planner (development aid; bench.py does not cover it).

B rows with the settings of fixture cases 1 and 2 (tests/golden/paths.json) at dt = 0.001, the time step of the
reference's control loops.  HIP events on the planner's stream, 3 warm-up and 10 timed calls per figure; prints ONE JSON
line:
  plan_us / fill_gradient_us   engine.path_plan (with its read-back of the step counts' inputs) and engine.path_fill
                               (fill + gradient kernels) on device-resident rows; the split between the fill and the
                               gradient kernel comes from `rocprofv3 --kernel-trace --stats -- python tools/path_timing.py`
  generate_path_wall_ms        PathPlanner.generate_path(to_host=False): tables on the host, uploads, both passes
  path_bytes, fill_gradient_GBps   B x Tmax x 12 x 8 bytes of output and that over fill_gradient_us
  path_next_graph_us           { path_next } recorded into a plan at B rows, launch_graph(2000), per tick
  reference_ms_per_path        the reference's own figure for the same case from the fixture JSON, with its CPU model

    python tools/path_timing.py [--rows 4096]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WARMUP, TIMED = 3, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    args = ap.parse_args()
    import abr_control_amd as a
    from abr_control_amd import _abi, engine
    from abr_control_amd.controllers.path_planners import PathPlanner
    from abr_control_amd.controllers.path_planners.path_planner import profile_tables
    from tests import path_cases

    meta, _ = path_cases.golden()
    B = args.rows
    s = a.Stream(0)

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

    res = {"device": a.device_name(0), "rows": B, "dt": 0.001, "warmup": WARMUP, "timed": TIMED, "cases": {},
           "reference_cpu": meta["cpu_model"]}
    for name in ("case1", "case2"):
        case = meta["cases"][name]
        r = np.random.RandomState(1)
        start = r.uniform(-0.4, 0.4, (B, 3))
        d = r.normal(size=(B, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        target = start + d * r.uniform(case["length"][0], case["length"][1], (B, 1))
        so, to = r.uniform(-1, 1, (B, 3)), r.uniform(-1, 1, (B, 3))
        pos, vel = path_cases.profiles(name, dt=0.001)
        kw = dict(max_velocity=1.0, start_velocity=case["start_velocity"], target_velocity=case["target_velocity"])
        planner = PathPlanner(pos, vel, stream=s)
        wall = []
        for _ in range(WARMUP + 5):
            t0 = time.perf_counter()
            planner.generate_path(start, target, start_orientation=so, target_orientation=to, to_host=False, **kw)
            s.sync()
            wall.append(1e3 * (time.perf_counter() - t0))
        nt = planner.n_timesteps
        t_max = int(nt.max())
        # the two passes on device-resident rows
        table, off, cands = profile_tables(pos, vel, **kw)
        P = _abi.PathParams(0.001, pos.n_sample_points, len(cands), 22, 12, table.size)
        up = lambda x: a.DeviceArray.from_numpy(np.ascontiguousarray(x), 0, s.ptr)
        d_table, d_start, d_target, d_so, d_to = (up(x) for x in (table, start, target, so, to))
        nt_d, rp_d, ds_d = engine.path_plan(P, d_table, off, d_start, d_target, stream=s)
        out = a.DeviceArray((B, t_max, 12))
        plan = timed(lambda: engine.path_plan(P, d_table, off, d_start, d_target, stream=s))
        fill = timed(lambda: engine.path_fill(P, d_table, off, t_max, d_start, d_target, nt_d, rp_d, ds_d, d_so, d_to,
                                              path=out, stream=s))
        nbytes = B * t_max * 12 * 8
        # the feed of a recorded loop
        counter = a.DeviceArray((B,), np.int32).zero_(s)
        tgt, tv = a.DeviceArray((B, 6)).zero_(s), a.DeviceArray((B, 6)).zero_(s)
        with engine.Plan(device=0, stream=s) as tick:
            engine.path_next(out, nt_d, counter, tgt, tv, stream=s)
        nxt = timed(lambda: tick.launch_graph(2000), launches=5, per=2000)
        res["cases"][name] = {
            "n_sample_points": pos.n_sample_points, "steps": [int(nt.min()), int(np.median(nt)), t_max],
            "plan_us": plan, "fill_gradient_us": fill, "generate_path_wall_ms": float(np.median(wall[WARMUP:])),
            "path_bytes": nbytes, "valid_bytes": int(nt.sum()) * 96,
            "fill_gradient_GBps": nbytes / fill["median_us"] / 1e3, "path_next_graph_us": nxt,
            "reference_ms_per_path": meta["reference_ms_per_path_dt0.001"][name]["ms"]}
        del out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
