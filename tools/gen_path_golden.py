#!/usr/bin/env python3
"""Fixtures of the batched path planner (tests/golden/paths.{npz,json}) by RUNNING THE REFERENCE'S OWN PathPlanner.

TEST INFRASTRUCTURE - not part of the product.  Runs where the reference is importable (a scratch copy of it is made
by oracle/gen_golden.py's make_scratch, as for the other fixtures, and MPLBACKEND=Agg keeps its matplotlib import
headless); the GPU box only ever sees the committed files.

paths.json holds the settings of every case (profile classes and their arguments, dt, velocities, axes), the reference's
measured milliseconds per path with the CPU model (the speed baseline of DESIGN.md "Path planner"), and what was
observed about the knife edges; paths.npz holds per case the rows' start / target positions and Euler angles, the
reference's paths (rows concatenated along time, `n_timesteps` cuts them), the sampled position profile and the
velocity ramps `vel_profile.generate` returned for every candidate max_v a row tried.

Every row must stay clear of the branches a last-bit difference could flip, or generation FAILS (nothing is redrawn
silently): int(remaining / max_v / dt) at least 1e-6 from an integer; |curve_length - (starting_dist + ending_dist)| at
least 1e-9 for every candidate tried, rejected ones included; every Euler angle on the path below 2.5 in magnitude and
the middle one below 1.4 (away from wrap-around and gimbal lock).

Usage:  python tools/gen_path_golden.py
"""
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
DT = 0.004
ROWS = 6

CASES = {
    "case1": dict(pos=["Linear", {}], vel=["Gaussian", {"acceleration": 4}], start_velocity=0, target_velocity=0,
                  length=[0.25, 0.6]),
    "case2": dict(pos=["SinCurve", {"axes": ["x", "z"], "cycles": [1, 1, 2], "n_sample_points": 200}],
                  vel=["Linear", {"acceleration": 4}], start_velocity=0.1, target_velocity=0, length=[0.25, 0.6]),
    "case3": dict(pos=["Ellipse", {"horz_stretch": 0.5, "n_sample_points": 200}], vel=["Gaussian", {"acceleration": 3}],
                  start_velocity=0, target_velocity=0.2, length=[0.25, 0.6]),
    "case4": dict(pos=["Linear", {}], vel=["Linear", {"acceleration": 4}], start_velocity=0, target_velocity=0,
                  length=[0.02, 0.12]),
    # one 6-wide case (no orientation), one in the reference's default axes, one FromPoints profile (1-2 rows each)
    "wide6": dict(pos=["Linear", {}], vel=["Gaussian", {"acceleration": 4}], start_velocity=0, target_velocity=0,
                  length=[0.2, 0.26], rows=2, orientation=False),
    "sxyz": dict(pos=["Linear", {}], vel=["Linear", {"acceleration": 4}], start_velocity=0, target_velocity=0,
                 length=[0.2, 0.26], rows=1, axes="sxyz"),
    "frompoints": dict(pos=["FromPoints", {"n_sample_points": 100}], vel=["Gaussian", {"acceleration": 4}],
                       start_velocity=0, target_velocity=0, length=[0.2, 0.26], rows=1),
}
FROM_POINTS_X = np.linspace(0, 1, 5)
FROM_POINTS_Y = np.array([[0, 0.3, 0.45, 0.8, 1], [0, 0.2, 0.6, 0.7, 1], [0, 0.25, 0.5, 0.75, 1]], dtype=float)


def make_profiles(case, pp, vp, dt):
    """the profile objects of a case from the modules pp (position_profiles) and vp (velocity_profiles)"""
    name, kw = case["pos"]
    kw = json.loads(json.dumps(kw))  # fresh lists: SinCurve rewrites `cycles` in place
    if name == "FromPoints":
        pos = pp.FromPoints(FROM_POINTS_X, FROM_POINTS_Y, **kw)
    else:
        pos = getattr(pp, name)(**kw)
    name, kw = case["vel"]
    return pos, getattr(vp, name)(dt=dt, **kw)


def draw_rows(rng, case):
    n = case.get("rows", ROWS)
    start = rng.uniform(-0.4, 0.4, (n, 3))
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    length = rng.uniform(case["length"][0], case["length"][1], (n, 1))
    return start, start + direction * length, rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3))


def worker(out_npz, out_json):
    from abr_control.controllers.path_planners import position_profiles as pp
    from abr_control.controllers.path_planners import velocity_profiles as vp
    from abr_control.controllers.path_planners.orientation import Orientation
    from abr_control.controllers.path_planners.path_planner import PathPlanner
    from abr_control.utils import transformations

    rng = np.random.RandomState(1234)
    out, meta = {}, {"dt": DT, "max_velocity": 1.0, "cases": {}, "observed": {}}
    cpu = [ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")]
    meta["cpu_model"] = cpu[0] if cpu else "unknown"
    for name, case in CASES.items():
        axes = case.get("axes", "rxyz")
        with_ori = case.get("orientation", True)
        start, target, so, to = draw_rows(rng, case)
        pos, vel = make_profiles(case, pp, vp, DT)
        planner = PathPlanner(pos, vel, axes=axes)
        paths, nts, finals, kmax, t_ms = [], [], [], 0, []
        int_gap, branch_gap, euler_max, mid_max = np.inf, np.inf, 0.0, 0.0
        for b in range(len(start)):
            t0 = time.perf_counter()
            path = planner.generate_path(start[b], target[b], 1.0, start_orientation=so[b] if with_ori else None,
                                         target_orientation=to[b] if with_ori else None,
                                         start_velocity=case["start_velocity"], target_velocity=case["target_velocity"])
            t_ms.append(1e3 * (time.perf_counter() - t0))
            # the search of path_planner.py:242-302 once more, to see how close every decision was
            chords = np.linalg.norm(np.diff(planner.warped_xyz, axis=0), axis=1)
            curve_length = np.sum(np.concatenate([[0], chords]))
            max_v, k = 1.0, 0
            while True:
                assert max_v > 0
                sp = vel.generate(start_velocity=case["start_velocity"], target_velocity=max_v)
                ep = sp[::-1] if case["start_velocity"] == case["target_velocity"] else vel.generate(
                    start_velocity=case["target_velocity"], target_velocity=max_v)[::-1]
                sd, ed = np.sum(sp * DT), np.sum(ep * DT)
                gap = abs(curve_length - (sd + ed))
                assert gap >= 1e-9, f"{name} row {b}: candidate {k} sits on the branch ({gap})"
                branch_gap = min(branch_gap, gap)
                if curve_length > sd + ed:
                    steps = (curve_length - (ed + sd)) / max_v / DT
                    d = abs(steps - np.round(steps))
                    assert d >= 1e-6, f"{name} row {b}: {steps} constant-speed steps sit on an integer"
                    int_gap = min(int_gap, d)
                    assert len(sp) + int(steps) + len(ep) == len(path) == planner.n_timesteps
                    break
                max_v -= 0.1
                k += 1
            kmax = max(kmax, k)
            finals.append(max_v)
            if with_ori:
                ang = np.abs(path[:, 6:9])
                assert ang.max() < 2.5 and ang[:, 1].max() < 1.4, f"{name} row {b}: Euler angles near a wrap"
                euler_max, mid_max = max(euler_max, ang.max()), max(mid_max, ang[:, 1].max())
            paths.append(path)
            nts.append(len(path))
        out[f"{name}_start"], out[f"{name}_target"] = start, target
        out[f"{name}_start_orientation"], out[f"{name}_target_orientation"] = so, to
        out[f"{name}_path"] = np.concatenate(paths, axis=0)
        out[f"{name}_n_timesteps"] = np.array(nts, dtype=np.int32)
        out[f"{name}_samples"] = np.array([pos.step(t) for t in np.linspace(0, 1, pos.n_sample_points)], dtype=float)
        max_v = 1.0
        for k in range(kmax + 1):
            out[f"{name}_ramp_start_{k}"] = vel.generate(start_velocity=case["start_velocity"], target_velocity=max_v)
            out[f"{name}_ramp_target_{k}"] = vel.generate(start_velocity=case["target_velocity"], target_velocity=max_v)
            max_v -= 0.1
        meta["cases"][name] = dict(case, axes=axes, orientation=with_ori, rows=len(start), candidates_stored=kmax + 1)
        meta["observed"][name] = dict(n_timesteps=[int(min(nts)), int(max(nts))], final_max_v=[min(finals), max(finals)],
                                      integer_gap_min=float(int_gap), branch_gap_min=float(branch_gap),
                                      euler_abs_max=float(euler_max), middle_angle_abs_max=float(mid_max),
                                      reference_ms_per_path=float(np.median(t_ms)))
        print(f"  {name}: T {min(nts)}..{max(nts)}, max_v {min(finals):.1f}..{max(finals):.1f}, int gap {int_gap:.3g}, "
              f"branch gap {branch_gap:.3g}, {np.median(t_ms):.1f} ms/path", flush=True)
    out["frompoints_x"], out["frompoints_y"] = FROM_POINTS_X, FROM_POINTS_Y

    # the speed baseline of tools/path_timing.py: the reference at dt = 0.001 on the first three rows of cases 1 and 2
    meta["reference_ms_per_path_dt0.001"] = {}
    for name in ("case1", "case2"):
        case = CASES[name]
        pos, vel = make_profiles(case, pp, vp, 0.001)
        planner = PathPlanner(pos, vel)
        t_ms, steps = [], []
        for b in range(3):
            t0 = time.perf_counter()
            p = planner.generate_path(out[f"{name}_start"][b], out[f"{name}_target"][b], 1.0,
                                      start_orientation=out[f"{name}_start_orientation"][b],
                                      target_orientation=out[f"{name}_target_orientation"][b],
                                      start_velocity=case["start_velocity"], target_velocity=case["target_velocity"])
            t_ms.append(1e3 * (time.perf_counter() - t0))
            steps.append(len(p))
        meta["reference_ms_per_path_dt0.001"][name] = dict(ms=float(np.median(t_ms)), steps=steps)
        print(f"  {name} at dt=0.001: {np.median(t_ms):.0f} ms/path, {steps} steps", flush=True)

    # Orientation(n_timesteps=50).generate_path in both output formats
    q0 = transformations.quaternion_from_euler(0.3, -0.5, 0.8, axes="rxyz")
    q1 = transformations.quaternion_from_euler(-0.6, 0.4, -0.2, axes="rxyz")
    out["orientation_q0"], out["orientation_q1"] = np.array(q0), np.array(q1)
    for fmt in ("euler", "quaternion"):
        out[f"orientation_{fmt}"] = np.array(Orientation(n_timesteps=50, output_format=fmt).generate_path(q0, q1))
    np.savez_compressed(out_npz, **out)
    with open(out_json, "w") as fh:
        json.dump(meta, fh, indent=1)
        fh.write("\n")
    print(f"  wrote {out_npz} ({os.path.getsize(out_npz)} bytes) and {out_json}", flush=True)
    assert os.path.getsize(out_npz) <= 600 * 1000


def main():
    if sys.argv[1:2] == ["--worker"]:
        return worker(*sys.argv[2:4])
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    from gen_golden import make_scratch

    scratch = make_scratch()
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=scratch, MPLBACKEND="Agg")
    try:
        subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", os.path.join(OUT, "paths.npz"),
                        os.path.join(OUT, "paths.json")], env=env, check=True)
    finally:
        shutil.rmtree(os.path.dirname(scratch), ignore_errors=True)


if __name__ == "__main__":
    main()
