"""The path planner's fixture cases (tests/golden/paths.{npz,json}, written by tools/gen_path_golden.py from the
reference's own PathPlanner), loaded once and shared by the path planner tests."""
import functools
import json
import os

import numpy as np

from abr_control_amd.controllers.path_planners import position_profiles, velocity_profiles

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# The project's bar for planner outputs (tests/test_gpu_parity.py test_gpu_inverse_kinematics): absolute, on all columns.
# Counts and branches are exact by construction of the fixtures; positions and angles differ from the reference by
# summation order and a few ulps of sin / acos / atan2, the gradient columns by 1 / (2 dt) = 125 times that.
BOUND = 1e-9
MAIN = ("case1", "case2", "case3", "case4")


@functools.lru_cache(maxsize=None)
def golden():
    meta = json.load(open(os.path.join(_GOLDEN, "paths.json")))
    data = dict(np.load(os.path.join(_GOLDEN, "paths.npz")))
    for v in data.values():
        v.setflags(write=False)
    return meta, data


def names():
    return list(golden()[0]["cases"])


def profiles(name, dt=None):
    """fresh profile objects of a case (this package's classes)"""
    meta, data = golden()
    case = meta["cases"][name]
    kind, kw = case["pos"]
    kw = json.loads(json.dumps(kw))
    if kind == "FromPoints":
        pos = position_profiles.FromPoints(data["frompoints_x"], data["frompoints_y"], **kw)
    else:
        pos = getattr(position_profiles, kind)(**kw)
    kind, kw = case["vel"]
    return pos, getattr(velocity_profiles, kind)(dt=meta["dt"] if dt is None else dt, **kw)


def rows(name):
    """-> dict(start, target, so, to (None for a 6-wide case), nt, paths: list of the reference's [T, W] paths,
    kwargs: max_velocity / start_velocity / target_velocity, axes)"""
    meta, data = golden()
    case = meta["cases"][name]
    nt = data[f"{name}_n_timesteps"]
    cuts = np.cumsum(nt)[:-1]
    ori = case["orientation"]
    return dict(start=data[f"{name}_start"], target=data[f"{name}_target"],
                so=data[f"{name}_start_orientation"] if ori else None,
                to=data[f"{name}_target_orientation"] if ori else None, nt=nt,
                paths=np.split(data[f"{name}_path"], cuts, axis=0), axes=case["axes"],
                kwargs=dict(max_velocity=meta["max_velocity"], start_velocity=case["start_velocity"],
                            target_velocity=case["target_velocity"]))


def check_against_reference(name, path, nt, report):
    """path [B, Tmax, W], nt [B] of any implementation against the fixture: counts exact, values within BOUND on every
    column, padding equal to the row's last point.  report(column group, max abs difference) gets the figures first."""
    r = rows(name)
    assert np.array_equal(np.asarray(nt), r["nt"]), (name, nt, r["nt"])
    worst = np.zeros(path.shape[-1])
    for b, ref in enumerate(r["paths"]):
        T = len(ref)
        worst = np.maximum(worst, np.abs(path[b, :T] - ref).max(axis=0))
        assert np.array_equal(path[b, T:], np.broadcast_to(path[b, T - 1], path[b, T:].shape)), (name, b, "padding")
    for lo, label in ((0, "position"), (3, "velocity"), (6, "euler"), (9, "angular velocity")):
        if lo < len(worst):
            report(f"{name} {label}", worst[lo:lo + 3].max())
    assert worst.max() < BOUND, (name, worst)
