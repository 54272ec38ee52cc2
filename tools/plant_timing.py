#!/usr/bin/env python3
"""Timing of the rigid-body plant step on UR5 fp64 (development aid; bench.py does not cover the plant).

HIP events on the launch stream, 12 warm-up and 30 timed launches per figure; prints ONE JSON line:
  plant_us[rows][substeps]      plant_step alone at 4096 and 8 M rows, substeps 1 and 100
  osc_cfg4_us[rows]             the x,y,z + use_C + use_g OSC kernel alone, same process
  tick_graph_us                 the recorded {OSC cfg4; plant step} tick at 4096 rows, launch_graph(2000), per tick

    python tools/plant_timing.py [--rows-large 8388608]

--effects: the plant with non-ideal effects against the plain step, in one process (profiles/plant_step.md): UR5 and
Jaco2 fp64 at 4096 and 1 M rows, one step of 1 ms - plain entry point, effects entry point with nothing switched on,
and with everything on (saturation, tau_ext, wrench, viscous and Coulomb friction, limits).  The three are timed in turn,
five rounds of 12 warm-up + 30 timed launches each; the figure is the median over all 150 launches, the ratio is to the
plain step of the same rounds.  Prints ONE JSON line.

    python tools/plant_timing.py --effects [--rows-fx 1048576]

--payload: the same leg with the payload step beside them (profiles/plant_step.md): plain entry point, effects entry
point with everything on, payload entry point with nothing else, and with everything on; payloads of 0.2 - 3 kg within
10 cm of the end effector, every seventh row without a mass.  Same rounds, same table form, ratios to the plain step.

    python tools/plant_timing.py --payload [--rows-fx 1048576]

--contact: the contact kernel beside the plain plant step (profiles/contact_step.md): UR5 and Jaco2, fp64 and fp32, at
4096 and 1 M rows - contact.contact_step with one and with four surfaces per row and the report on, a third of the rows
pressing, a third clear, a third leaving; and, at 4096 rows, the recorded tick { contact; plant_step(tau_ext) } against
{ plant_step } per replayed tick.  Same rounds; ratios to the plain step of the same rounds.  bytes_per_row is what the
kernel reads and writes (q, dq, S surfaces, tau, report), gbytes_per_s that over the median.

    python tools/plant_timing.py --contact [--rows-fx 1048576]

--force: the force-control law beside the contact step and the plain plant step of the same run
(profiles/force_control.md): UR5 and Jaco2, fp64 and fp32, at 4096 and 1 M rows - ForceController.generate reading a
[B,8] report, two rows in three in contact (every third free), every option on; contact.contact_step with one surface
and the report on; and, at 4096 rows, the recorded tick { force law; contact; plant_step(tau_ext) } against
{ plant_step } per replayed tick.  The protocol of --contact: same rounds, ratios to the plain step of the same rounds.

    python tools/plant_timing.py --force [--rows-fx 1048576]

--links: the whole-arm contact step beside what it replaces, in the same run (profiles/link_contact.md): UR5 and Jaco2,
fp64 and fp32, at 4096 and 1 M rows - Obstacles.apply with K = 1, 4 and 8 spheres per row and the report on, every link
segment a capsule of 40 mm, the spheres placed at the middle of the row's own segments so that about two rows in three
touch (the share is in the output); (a) contact.contact_step with four surfaces; (b) N contact_step calls, one per link
frame, the later ones with accumulate - covering the links with points, as include/abrk.h advised before.  The protocol
of --contact: same rounds; ratio_to_contact_s4 and ratio_to_n_calls are to those two of the same rounds.

    python tools/plant_timing.py --links [--rows-fx 1048576]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP, TIMED = 12, 30


def effects_leg(rows_large, payload=False):
    import abr_control_amd as a
    from abr_control_amd import _abi, engine, plant_payload
    from abr_control_amd.arms import jaco2, ur5

    s = a.Stream(0)
    p = _abi.make_plant_params(1e-3)
    res = {"leg": "payload" if payload else "effects", "dtype": "float64", "device": a.device_name(0), "warmup": WARMUP, "timed": TIMED,
           "rounds": 5, "us": {}}
    e0, e1 = a.Event(0), a.Event(0)

    def one_round(fn):
        for _ in range(WARMUP):
            fn()
        s.sync()
        ts = []
        for _ in range(TIMED):
            e0.record(s)
            fn()
            e1.record(s)
            s.sync()
            ts.append(e1.elapsed_ms_since(e0) * 1e3)
        return ts

    for name, rc in (("ur5", ur5.Config()), ("jaco2", jaco2.Config())):
        n = rc.N_JOINTS
        all_on = _abi.make_plant_effects(n, damping=0.5, coulomb=0.3, coulomb_vs=0.01, tau_max=12.0, q_min=-2.0,
                                         q_max=2.0, restitution=0.5)
        all_off = _abi.make_plant_effects(n)
        res["us"][name] = {}
        for B in (4096, rows_large):
            rng = np.random.RandomState(0)
            q0, dq0 = rng.uniform(-1.9, 1.9, (B, n)), rng.uniform(-2, 2, (B, n))
            u, ext, w = (a.DeviceArray.from_numpy(x) for x in (rng.uniform(-20, 20, (B, n)), rng.uniform(-5, 5, (B, n)),
                                                               rng.uniform(-10, 10, (B, 6))))
            q, dq = a.DeviceArray.from_numpy(q0), a.DeviceArray.from_numpy(dq0)
            load = np.concatenate([rng.uniform(0.2, 3.0, (B, 1)), rng.uniform(-0.1, 0.1, (B, 3))], axis=1)
            load[::7, 0] = 0
            pl = a.DeviceArray.from_numpy(load) if payload else None

            def reset():  # every round starts from the same state: the three forms see the same rows
                q.copy_from_numpy(q0, stream=s)
                dq.copy_from_numpy(dq0, stream=s)
                s.sync()

            forms = {
                "plain": lambda: engine.plant_step(rc.arm_id, n, p, q, dq, u, stream=s),
                "fx_all_off": lambda: engine.plant_step(rc.arm_id, n, p, q, dq, u, stream=s, effects=all_off),
                "fx_all_on": lambda: engine.plant_step(rc.arm_id, n, p, q, dq, u, stream=s, effects=all_on, tau_ext=ext,
                                                       wrench=w),
            }
            if payload:
                forms = {
                    "plain": forms["plain"],
                    "fx_all_on": forms["fx_all_on"],
                    "payload_alone": lambda: plant_payload.plant_step(rc.arm_id, n, p, q, dq, u, stream=s,
                                                                      payload=pl),
                    "payload_all_on": lambda: plant_payload.plant_step(rc.arm_id, n, p, q, dq, u, stream=s,
                                                                       effects=all_on, tau_ext=ext, wrench=w,
                                                                       payload=pl),
                }
            ts = {k: [] for k in forms}
            for _ in range(res["rounds"]):
                for k, fn in forms.items():
                    reset()
                    ts[k] += one_round(fn)
            out = {k: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))}
                   for k, v in ts.items()}
            for k in forms:
                if k == "plain":
                    continue
                out[k]["ratio_to_plain"] = out[k]["median_us"] / out["plain"]["median_us"]
            res["us"][name][str(B)] = out
    print(json.dumps(res))


def contact_leg(rows_large):
    import abr_control_amd as a
    from abr_control_amd import _abi, contact, engine
    from abr_control_amd.arms import jaco2, ur5

    s = a.Stream(0)
    p = _abi.make_plant_params(1e-3)
    rounds = 5
    res = {"leg": "contact", "device": a.device_name(0), "warmup": WARMUP, "timed": TIMED, "rounds": rounds, "us": {}}
    e0, e1 = a.Event(0), a.Event(0)

    def one_round(fn, per=1):
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
        return ts

    for name, make in (("ur5", ur5.Config), ("jaco2", jaco2.Config)):
        res["us"][name] = {}
        for dtype in (np.float64, np.float32):
            rc = make(dtype=dtype)
            n = rc.N_JOINTS
            res["us"][name][np.dtype(dtype).name] = {}
            for B in (4096, rows_large):
                rng = np.random.RandomState(0)
                q0, dq0 = rng.uniform(-1.9, 1.9, (B, n)).astype(dtype), rng.uniform(-2, 2, (B, n)).astype(dtype)
                q, dq = a.DeviceArray.from_numpy(q0), a.DeviceArray.from_numpy(dq0)
                u = a.DeviceArray.from_numpy(rng.uniform(-20, 20, (B, n)).astype(dtype))
                # planes through each row's own point: delta = +25 mm (two rows in three) or -25 mm; of the penetrated
                # ones every other is left faster than its spring pushes (c vn > k delta)
                xyz = np.asarray(rc.Tx("EE", q0), dtype=np.float64)
                v = np.einsum("bij,bj->bi", np.asarray(rc.J("EE", q0), dtype=np.float64)[:, :3], dq0.astype(np.float64))
                tables = {}
                for S in (1, 4):
                    nrm = rng.normal(size=(B, S, 3))
                    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
                    delta = np.where(np.arange(B) % 3 == 1, -0.025, 0.025)[:, None] * np.ones((1, S))
                    planes = np.zeros((B, S, 8))
                    planes[:, :, :3] = nrm
                    planes[:, :, 3] = np.einsum("bsi,bi->bs", nrm, xyz) + delta
                    planes[:, :, 4:] = [2e4, 100.0, 0.5, 0.0]
                    planes[2::3, :, 5] = 500.0
                    tables[S] = a.ContactSurfaces(rc, B, planes.astype(dtype).astype(np.float64), stream=s)

                def reset():
                    q.copy_from_numpy(q0, stream=s)
                    dq.copy_from_numpy(dq0, stream=s)
                    s.sync()

                forms = {
                    "plain": lambda: engine.plant_step(rc.arm_id, n, p, q, dq, u, dtype=dtype, stream=s),
                    "contact_s1": lambda: tables[1].apply(q, dq),
                    "contact_s4": lambda: tables[4].apply(q, dq),
                }
                ts = {k: [] for k in forms}
                for _ in range(rounds):
                    for k, fn in forms.items():
                        reset()
                        ts[k] += one_round(fn)
                if B == 4096:
                    with engine.Plan(device=0, stream=s) as bare:
                        engine.plant_step(rc.arm_id, n, p, q, dq, u, dtype=dtype, stream=s)
                    with engine.Plan(device=0, stream=s) as tick:
                        tau = tables[1].apply(q, dq)
                        engine.plant_step(rc.arm_id, n, p, q, dq, u, dtype=dtype, stream=s, tau_ext=tau)
                    for k, plan in (("tick_plant_graph", bare), ("tick_contact_plant_graph", tick)):
                        reset()
                        ts[k] = one_round(lambda: plan.launch_graph(200), per=200)[:10]
                out = {k: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))}
                       for k, v in ts.items()}
                esz = np.dtype(dtype).itemsize
                for k, S in (("contact_s1", 1), ("contact_s4", 4)):
                    out[k]["ratio_to_plain"] = out[k]["median_us"] / out["plain"]["median_us"]
                    out[k]["bytes_per_row"] = (3 * n + 8 * S + 8) * esz
                    out[k]["gbytes_per_s"] = out[k]["bytes_per_row"] * B / out[k]["median_us"] * 1e-3
                if B == 4096:
                    out["tick_contact_plant_graph"]["added_us"] = (out["tick_contact_plant_graph"]["median_us"]
                                                                   - out["tick_plant_graph"]["median_us"])
                res["us"][name][np.dtype(dtype).name][str(B)] = out
    print(json.dumps(res))


def links_leg(rows_large):
    import abr_control_amd as a
    from abr_control_amd import _abi, contact
    from abr_control_amd.arms import jaco2, ur5

    s = a.Stream(0)
    rounds = 5
    res = {"leg": "links", "device": a.device_name(0), "warmup": WARMUP, "timed": TIMED, "rounds": rounds, "us": {}}
    e0, e1 = a.Event(0), a.Event(0)

    def one_round(fn):
        for _ in range(WARMUP):
            fn()
        s.sync()
        ts = []
        for _ in range(TIMED):
            e0.record(s)
            fn()
            e1.record(s)
            s.sync()
            ts.append(e1.elapsed_ms_since(e0) * 1e3)
        return ts

    for name, make in (("ur5", ur5.Config), ("jaco2", jaco2.Config)):
        res["us"][name] = {}
        for dtype in (np.float64, np.float32):
            rc = make(dtype=dtype)
            n = rc.N_JOINTS
            res["us"][name][np.dtype(dtype).name] = {}
            for B in (4096, rows_large):
                rng = np.random.RandomState(0)
                q0, dq0 = rng.uniform(-1.9, 1.9, (B, n)).astype(dtype), rng.uniform(-2, 2, (B, n)).astype(dtype)
                q, dq = a.DeviceArray.from_numpy(q0), a.DeviceArray.from_numpy(dq0)
                ends = [np.asarray(rc.Tx(f"joint{i}", q0), dtype=np.float64) for i in range(n)]
                ends.append(np.asarray(rc.Tx("EE", q0), dtype=np.float64))

                def plane_table(frame, S, point):
                    # planes through each row's own point, as in the --contact leg: delta = +-25 mm
                    nrm = rng.normal(size=(B, S, 3))
                    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
                    delta = np.where(np.arange(B) % 3 == 1, -0.025, 0.025)[:, None] * np.ones((1, S))
                    planes = np.zeros((B, S, 8))
                    planes[:, :, :3] = nrm
                    planes[:, :, 3] = np.einsum("bsi,bi->bs", nrm, point) + delta
                    planes[:, :, 4:] = [2e4, 100.0, 0.5, 0.0]
                    return a.ContactSurfaces(rc, B, planes.astype(dtype).astype(np.float64), frame=frame, stream=s)

                s4 = plane_table("EE", 4, ends[n])
                per_link = [plane_table(f"link{i + 1}", 1, np.asarray(rc.Tx(f"link{i + 1}", q0), dtype=np.float64))
                            for i in range(n)]
                worlds = {}
                for K in (1, 4, 8):
                    # sphere o of a row at the middle of segment (o + row) % n, its centre R + r -+ 25 mm from the axis
                    obs = np.zeros((B, K, 7))
                    for o in range(K):
                        seg = (o + np.arange(B)) % n
                        mid = np.stack([0.5 * (ends[i] + ends[i + 1]) for i in range(n)])[seg, np.arange(B)]
                        d = rng.normal(size=(B, 3))
                        d /= np.linalg.norm(d, axis=1, keepdims=True)
                        delta = np.where(np.arange(B) % 3 == 1, -0.025, 0.025)
                        obs[:, o, :3] = mid + d * (0.05 + 0.04 - delta)[:, None]
                        obs[:, o, 3:] = [0.05, 2e4, 100.0, 0.5]
                    worlds[K] = a.Obstacles(rc, B, obs.astype(dtype).astype(np.float64), link_radius=0.04, stream=s)

                def n_calls():
                    tau = per_link[0].apply(q, dq)
                    for t in per_link[1:]:
                        t.apply(q, dq, tau=tau, accumulate=True)

                forms = {"contact_s4": lambda: s4.apply(q, dq), "contact_n_calls": n_calls}
                for K in worlds:
                    forms[f"links_k{K}"] = (lambda w: lambda: w.apply(q, dq))(worlds[K])
                ts = {k: [] for k in forms}
                for _ in range(rounds):
                    for k, fn in forms.items():
                        ts[k] += one_round(fn)
                out = {k: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))}
                       for k, v in ts.items()}
                esz = np.dtype(dtype).itemsize
                for K in worlds:
                    o = out[f"links_k{K}"]
                    o["ratio_to_contact_s4"] = o["median_us"] / out["contact_s4"]["median_us"]
                    o["ratio_to_n_calls"] = o["median_us"] / out["contact_n_calls"]["median_us"]
                    o["bytes_per_row"] = (3 * n + 7 * K + 8) * esz
                    o["gbytes_per_s"] = o["bytes_per_row"] * B / o["median_us"] * 1e-3
                    o["rows_touching"] = float((worlds[K].report()["n_contacts"] > 0).mean())
                res["us"][name][np.dtype(dtype).name][str(B)] = out
    print(json.dumps(res))


def force_leg(rows_large):
    import abr_control_amd as a
    from abr_control_amd import _abi, engine
    from abr_control_amd.arms import jaco2, ur5

    s = a.Stream(0)
    p = _abi.make_plant_params(1e-3)
    rounds = 5
    res = {"leg": "force", "device": a.device_name(0), "warmup": WARMUP, "timed": TIMED, "rounds": rounds, "us": {}}
    e0, e1 = a.Event(0), a.Event(0)

    def one_round(fn, per=1):
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
        return ts

    for name, make in (("ur5", ur5.Config), ("jaco2", jaco2.Config)):
        res["us"][name] = {}
        for dtype in (np.float64, np.float32):
            rc = make(dtype=dtype)
            n = rc.N_JOINTS
            res["us"][name][np.dtype(dtype).name] = {}
            for B in (4096, rows_large):
                rng = np.random.RandomState(0)
                q0, dq0 = rng.uniform(-1.9, 1.9, (B, n)).astype(dtype), rng.uniform(-2, 2, (B, n)).astype(dtype)
                q, dq = a.DeviceArray.from_numpy(q0), a.DeviceArray.from_numpy(dq0)
                u = a.DeviceArray.from_numpy(rng.uniform(-20, 20, (B, n)).astype(dtype))
                xyz = np.asarray(rc.Tx("EE", q0), dtype=np.float64)
                nrm = rng.normal(size=(B, 3))
                nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
                # the contact step of the --contact leg with one surface: delta = +-25 mm through each row's own point
                planes = np.zeros((B, 1, 8))
                planes[:, 0, :3] = nrm
                planes[:, 0, 3] = np.einsum("bi,bi->b", nrm, xyz) + np.where(np.arange(B) % 3 == 1, -0.025, 0.025)
                planes[:, 0, 4:] = [2e4, 100.0, 0.5, 0.0]
                table = a.ContactSurfaces(rc, B, planes.astype(dtype).astype(np.float64), stream=s)
                # the law: a sensed force of 2 - 30 N along n on two rows in three, none on the others
                sensed = np.zeros((B, 8))
                sensed[:, :3] = nrm.astype(dtype) * np.where(np.arange(B) % 3 == 1, 0.0, rng.uniform(2, 30, B))[:, None]
                report = a.DeviceArray.from_numpy(sensed.astype(dtype))
                tgt = np.zeros((B, 6))
                tgt[:, :3] = xyz + rng.uniform(-0.1, 0.1, (B, 3))
                tgt, tv = (a.DeviceArray.from_numpy(x.astype(dtype)) for x in (tgt, rng.uniform(-0.5, 0.5, (B, 6))))
                press = a.ForceController(rc, B, nrm.astype(dtype).astype(np.float64), rng.uniform(1, 40, B), dt=1e-3,
                                          stream=s)

                def reset():
                    q.copy_from_numpy(q0, stream=s)
                    dq.copy_from_numpy(dq0, stream=s)
                    press.reset()
                    s.sync()

                forms = {
                    "plain": lambda: engine.plant_step(rc.arm_id, n, p, q, dq, u, dtype=dtype, stream=s),
                    "contact_s1": lambda: table.apply(q, dq),
                    "force": lambda: press.generate(q, dq, tgt, report, target_velocity=tv),
                }
                ts = {k: [] for k in forms}
                for _ in range(rounds):
                    for k, fn in forms.items():
                        reset()
                        ts[k] += one_round(fn)
                if B == 4096:
                    with engine.Plan(device=0, stream=s) as bare:
                        engine.plant_step(rc.arm_id, n, p, q, dq, u, dtype=dtype, stream=s)
                    with engine.Plan(device=0, stream=s) as tick:
                        uf = press.generate(q, dq, tgt, table.device_arrays()["report"], target_velocity=tv)
                        tau = table.apply(q, dq)
                        engine.plant_step(rc.arm_id, n, p, q, dq, uf, dtype=dtype, stream=s, tau_ext=tau)
                    for k, plan in (("tick_plant_graph", bare), ("tick_force_contact_plant_graph", tick)):
                        reset()
                        ts[k] = one_round(lambda: plan.launch_graph(200), per=200)[:10]
                out = {k: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))}
                       for k, v in ts.items()}
                esz = np.dtype(dtype).itemsize
                for k in ("contact_s1", "force"):
                    out[k]["ratio_to_plain"] = out[k]["median_us"] / out["plain"]["median_us"]
                out["force"]["ratio_to_contact"] = out["force"]["median_us"] / out["contact_s1"]["median_us"]
                # q, dq, u; 3 of target, target_velocity and force each (their lines are fetched whole); cmd; integ twice
                out["force"]["bytes_per_row"] = (3 * n + 9 + 4 + 2) * esz
                out["force"]["gbytes_per_s"] = out["force"]["bytes_per_row"] * B / out["force"]["median_us"] * 1e-3
                if B == 4096:
                    out["tick_force_contact_plant_graph"]["added_us"] = (
                        out["tick_force_contact_plant_graph"]["median_us"] - out["tick_plant_graph"]["median_us"])
                res["us"][name][np.dtype(dtype).name][str(B)] = out
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-large", type=int, default=8 << 20)
    ap.add_argument("--effects", action="store_true", help="time the plant with effects against the plain step")
    ap.add_argument("--payload", action="store_true", help="time the payload step against the effects and the plain step")
    ap.add_argument("--contact", action="store_true", help="time the contact kernel against the plain step")
    ap.add_argument("--force", action="store_true", help="time the force-control law against the contact and plain steps")
    ap.add_argument("--links", action="store_true", help="time the whole-arm contact against the contact step and N of them")
    ap.add_argument("--rows-fx", type=int, default=1 << 20)
    args = ap.parse_args()
    if args.force:
        return force_leg(args.rows_fx)
    if args.contact:
        return contact_leg(args.rows_fx)
    if args.links:
        return links_leg(args.rows_fx)
    if args.effects or args.payload:
        return effects_leg(args.rows_fx, payload=args.payload)
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
