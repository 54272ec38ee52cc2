#!/usr/bin/env python3
"""Timing of the loop recorder on UR5 fp64 (development aid; bench.py does not cover it).  Prints ONE JSON line.

  tick_graph_us     4096 rows, the recorded { path_next; OSC x,y,z + g + C with target_velocity; plant_step } tick replayed
                    with launch_graph(K), per tick: "base"; "recorder" = + LoopRecorder.record (xyz + err history, statistics);
                    "dynamics_tx" = + engine.dynamics(want=("Tx",)), the only device-side way to the end-effector position
                    without the recorder.  12 warm-up replays of 100 ticks, 7 timed replays of K, medians.
  store_us          `--rows-large` rows, loop_trace alone, HIP events around `capacity` back-to-back launches (every launch
                    writes a fresh slot), 2 warm-up rounds and 7 timed: "all" = every column (W = 28), "xyz_err" = xyz + err
                    + statistics, "stats" = statistics only; with the history bytes per second and their share of
                    `--hbm-peak`.  The history store form is the library's default, or the row-per-lane form under
                    ABRK_MEASUREMENT=1 ABRK_TRACE_PLAIN=1 (a process reads the switch once: one run per form).
  d2d_copy_us       a device-to-device hipMemcpyAsync (torch) of the bytes one "all" slot takes: the ceiling of the stores

    python tools/trace_timing.py [--rows-large 1048576] [--ticks 1000]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-large", type=int, default=1 << 20)
    ap.add_argument("--ticks", type=int, default=1000)
    ap.add_argument("--capacity", type=int, default=8)
    ap.add_argument("--hbm-peak", type=float, default=8.0e12, help="bytes per second")
    args = ap.parse_args()
    import abr_control_amd as a
    from abr_control_amd import _abi, engine
    from abr_control_amd.arms import ur5
    from abr_control_amd.controllers.path_planners import PathPlanner, position_profiles, velocity_profiles

    rc = ur5.Config()
    n = 6
    s = a.Stream(0)
    e0, e1 = a.Event(0), a.Event(0)

    def timed(fn, per, warm, rounds, before=lambda: None):
        for _ in range(warm):
            before()
            fn()
        s.sync()
        ts = []
        for _ in range(rounds):
            before()
            e0.record(s)
            fn()
            e1.record(s)
            s.sync()
            ts.append(e1.elapsed_ms_since(e0) * 1e3 / per)
        return {"median_us": float(np.median(ts)), "min_us": float(np.min(ts)), "max_us": float(np.max(ts))}

    plain = os.environ.get("ABRK_MEASUREMENT") == "1" and os.environ.get("ABRK_TRACE_PLAIN") is not None
    res = {"arm": "ur5", "dtype": "float64", "device": a.device_name(0), "store_form": "row-per-lane" if plain else "lds",
           "tick_graph_us": {}, "store_us": {}}

    # ---- 4096 rows: the graph-replayed tick, launch-bound
    B, K = 4096, args.ticks
    rng = np.random.RandomState(0)
    q0 = rng.uniform(-1.0, 1.0, (B, n))
    planner = PathPlanner(position_profiles.Linear(), velocity_profiles.Gaussian(dt=0.001, acceleration=2), stream=s)
    planner.generate_path(rc.Tx("EE", q0), rc.Tx("EE", q0 + 0.2), max_velocity=1.0, start_orientation=np.zeros((B, 3)),
                          target_orientation=np.zeros((B, 3)), to_host=False)
    path, n_timesteps = planner.device_path()
    q, dq, u, tgt, tgt_v = (a.DeviceArray((B, w)) for w in (n, n, n, 6, 6))
    counter = a.DeviceArray((B,), np.int32)
    tx = a.DeviceArray((B, 3))
    law = _abi.make_osc_params(n, kp=200, use_C=True, use_g=True)
    plant = _abi.make_plant_params(0.001)
    rec = a.LoopRecorder(rc, B, capacity=K, columns=("xyz", "err"), stream=s)

    def restart():
        q.copy_from_numpy(q0, s)
        for arr in (dq, u, tgt, tgt_v, counter):
            arr.zero_(s)
        rec.reset()

    def plan(extra):
        with engine.Plan(device=0, stream=s) as tick:
            engine.path_next(path, n_timesteps, counter, tgt, tgt_v, stream=s)
            engine.osc_generate(rc.arm_id, n, law, q, dq, tgt, target_velocity=tgt_v, u=u, stream=s)
            engine.plant_step(rc.arm_id, n, plant, q, dq, u, stream=s)
            extra()
        return tick

    plans = {"base": plan(lambda: None), "recorder": plan(lambda: rec.record(q, dq, u, tgt)),
             "dynamics_tx": plan(lambda: engine.dynamics(rc.arm_id, n, q, want=("Tx",), out={"Tx": tx}, stream=s))}
    for _ in range(2):  # two passes in one process: the second shows the drift between identical measurements
        for name, tick in plans.items():
            restart()
            for _ in range(12):
                tick.launch_graph(100)
            r = timed(lambda: tick.launch_graph(K), K, 0, 7, before=restart)
            res["tick_graph_us"].setdefault(name, []).append(r)

    # ---- the store form at HBM-sized batches: loop_trace alone
    B, cap = args.rows_large, args.capacity
    qd, dqd, ud = (a.DeviceArray.from_numpy(rng.uniform(-1, 1, (B, n))) for _ in range(3))
    td = a.DeviceArray.from_numpy(rng.uniform(-1, 1, (B, 6)))
    for name, kw in (("all", dict(capacity=cap, columns=("q", "dq", "u", "target", "xyz", "err"))),
                     ("xyz_err", dict(capacity=cap, columns=("xyz", "err"))), ("stats", dict(capacity=0))):
        r = a.LoopRecorder(rc, B, stream=s, **kw)

        def launches(r=r):
            for _ in range(cap):
                r.record(qd, dqd, ud, td)

        t = timed(launches, cap, 2, 7, before=r.reset)
        t["history_bytes"] = B * r.W * 8 if r.device_history() is not None else 0
        t["history_GBps"] = t["history_bytes"] / t["median_us"] * 1e-3
        t["share_of_hbm_peak"] = t["history_bytes"] / (t["median_us"] * 1e-6) / args.hbm_peak
        res["store_us"][name] = t
        del r
    try:  # the ceiling: a device-to-device copy of one "all" slot
        import torch

        nb = B * 28 * 8
        src, dst = torch.empty(nb, dtype=torch.uint8, device="cuda"), torch.empty(nb, dtype=torch.uint8, device="cuda")
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for i in range(9):
            ev0.record()
            for _ in range(cap):
                dst.copy_(src, non_blocking=True)
            ev1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ts.append(ev0.elapsed_time(ev1) * 1e3 / cap)
        res["d2d_copy_us"] = {"bytes": nb, "median_us": float(np.median(ts)), "GBps_written": nb / np.median(ts) * 1e-3,
                              "share_of_hbm_peak": nb / (np.median(ts) * 1e-6) / args.hbm_peak}
    except ImportError:
        res["d2d_copy_us"] = None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
