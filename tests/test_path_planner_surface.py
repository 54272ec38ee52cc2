"""Python surface and C ABI of the path planner - no GPU needed: class names, signatures and defaults of the reference's
controllers/path_planners modules; every profile's step / generate bit for bit against the tables the reference's own
classes produced (tests/golden/paths.npz); Orientation against the reference's output; struct layout and argument
validation of abrk_path_plan_batch / _fill_batch / _next_batch before any device use."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from abr_control_amd import _abi
from abr_control_amd.controllers import path_planners
from abr_control_amd.controllers.path_planners import (Orientation, PathPlanner, position_profiles,
                                                        velocity_profiles)
from abr_control_amd.controllers.path_planners.path_planner import profile_tables
from tests import path_cases
from tests.conftest import REPO


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def test_surface_mirrors_reference():
    E = inspect.Parameter.empty
    pp, vp = position_profiles, velocity_profiles
    assert {"PosProf", "Linear", "SinCurve", "FromPoints", "Ellipse"} <= set(dir(pp))
    assert {"VelProf", "Gaussian", "Linear"} <= set(dir(vp))
    for name in ("InverseKinematics", "PathPlanner", "Orientation", "position_profiles", "velocity_profiles"):
        assert hasattr(path_planners, name)
    assert "run once per movement on the host" not in path_planners.__doc__
    assert _params(pp.PosProf.__init__)[:2] == [("tol", 1e-6), ("n_sample_points", 1000)]
    assert _params(pp.Linear.__init__)[0] == ("n_sample_points", 10)
    assert _params(pp.SinCurve.__init__)[:3] == [("axes", None), ("cycles", None), ("n_sample_points", 1000)]
    assert _params(pp.FromPoints.__init__)[:3] == [("x", E), ("y", E), ("n_sample_points", 1000)]
    assert _params(pp.Ellipse.__init__)[:3] == [("horz_stretch", E), ("plane", "xy"), ("n_sample_points", 1000)]
    assert _params(vp.VelProf.__init__) == [("dt", E)]
    assert _params(vp.Gaussian.__init__) == [("dt", E), ("acceleration", E), ("n_sigma", 3)]
    assert _params(vp.Linear.__init__) == [("dt", E), ("acceleration", E)]
    for cls in (vp.Gaussian, vp.Linear):
        assert _params(cls.generate) == [("start_velocity", E), ("target_velocity", E)]
    assert _params(Orientation.__init__) == [("n_timesteps", None), ("timesteps", None), ("axes", "rxyz"),
                                             ("output_format", "euler")]
    assert _params(Orientation.generate_path) == [("orientation", E), ("target_orientation", E), ("dr", None),
                                                  ("plot", False)]
    assert _params(Orientation.match_position_path) == [("orientation", E), ("target_orientation", E),
                                                        ("position_path", E), ("plot", False)]
    assert _params(PathPlanner.__init__)[:4] == [("pos_profile", E), ("vel_profile", E), ("axes", "rxyz"),
                                                 ("verbose", False)]
    assert _params(PathPlanner.generate_path)[:8] == [
        ("start_position", E), ("target_position", E), ("max_velocity", E), ("start_orientation", None),
        ("target_orientation", None), ("start_velocity", 0), ("target_velocity", 0), ("plot", False)]
    assert _params(PathPlanner.next_at_n) == [("n", E)]
    planner = PathPlanner(pp.Linear(), vp.Gaussian(dt=0.001, acceleration=1))
    assert (planner.n_sample_points, planner.dt, planner.n, planner.n_timesteps, planner.axes) == (10, 0.001, 0, None,
                                                                                                    "rxyz")
    assert planner.path.shape == (12, 1) and isinstance(planner.OrientationPlanner, Orientation)
    for m in ("generate_path", "next", "next_at_n", "device_path", "align_vectors"):
        assert callable(getattr(planner, m))
    with pytest.raises(NotImplementedError):
        Orientation(n_timesteps=5)._plot()
    with pytest.raises(NotImplementedError):
        planner.generate_path(np.zeros(3), np.ones(3), 1.0, plot=True)
    with pytest.raises(AssertionError):
        planner.generate_path(np.zeros(3), np.ones(3), 1.0, start_velocity=2.0)
    with pytest.raises(AssertionError):  # the end conditions of a profile are checked on construction
        type("Bad", (pp.PosProf,), {"step": lambda self, t: np.array([t, t, 2 * t])})()
    # SinCurve rewrites `cycles` in place, as the reference does
    cycles = [1, 1, 2]
    assert pp.SinCurve(["x", "z"], cycles).cycles is cycles and cycles == [1, 1, 5]


@pytest.mark.parametrize("name", path_cases.names())
def test_profiles_equal_the_reference_tables_bit_for_bit(name):
    meta, data = path_cases.golden(name)
    case = meta["cases"][name]
    pos, vel = path_cases.profiles(name)
    samples = np.array([pos.step(t) for t in np.linspace(0, 1, pos.n_sample_points)], dtype=float)
    assert np.array_equal(samples, data[f"{name}_samples"])
    max_v = meta["max_velocity"]
    table, offsets, cands = profile_tables(pos, vel, max_v, case["start_velocity"], case["target_velocity"])
    assert case["candidates_stored"] >= 1 and len(cands) >= case["candidates_stored"]
    for k in range(case["candidates_stored"]):
        up = vel.generate(start_velocity=case["start_velocity"], target_velocity=max_v)
        down = vel.generate(start_velocity=case["target_velocity"], target_velocity=max_v)
        assert np.array_equal(up, data[f"{name}_ramp_start_{k}"])
        assert np.array_equal(down, data[f"{name}_ramp_target_{k}"])
        # ... and the packed table holds exactly these: max_v by repeated subtraction, np.sum, np.cumsum, the mirror
        assert cands[k][0] == max_v and np.array_equal(cands[k][1], up) and np.array_equal(cands[k][2], down[::-1])
        o = offsets[2 + 4 * k:6 + 4 * k]
        assert np.array_equal(table[o[0]:o[0] + o[1]], np.cumsum(up * vel.dt)) and o[1] == len(up)
        assert np.array_equal(table[o[2]:o[2] + o[3]], np.cumsum(down[::-1] * vel.dt)) and o[3] == len(down)
        assert np.array_equal(table[offsets[1] + 3 * k:offsets[1] + 3 * k + 3],
                              [max_v, np.sum(up * vel.dt), np.sum(down[::-1] * vel.dt)])
        max_v -= 0.1
    assert np.array_equal(table[offsets[0]:offsets[0] + samples.size], samples.ravel())


def test_profile_tables_special_cases():
    """start_velocity == max_velocity / target_velocity == max_velocity (path_planner.py:153-163): a one-step ramp of
    v dt that covers no distance and is kept for every candidate; candidates stop where max_v <= 0; a user's own
    profile subclasses work"""
    vel = velocity_profiles.Linear(dt=0.01, acceleration=2)
    table, off, cands = profile_tables(position_profiles.Linear(), vel, 0.5, start_velocity=0.5, target_velocity=0.1)
    assert [c[3] for c in cands] == [0.0] * len(cands) and all(np.array_equal(c[1], [0.5 * 0.01]) for c in cands)
    expect, v = [], 0.5
    while v > 0:  # (0.5 - 5 x 0.1 leaves 2.8e-17 in floating point: a sixth candidate, as in the reference's loop)
        expect.append(v)
        v -= 0.1
    assert [c[0] for c in cands] == expect and len(expect) == 6
    assert off.shape == (2 + 4 * 6,) and off.dtype == np.int64
    _, _, cands = profile_tables(position_profiles.Linear(), vel, 0.5, start_velocity=0.0, target_velocity=0.5)
    assert all(c[4] == 0 and np.array_equal(c[2], [0.5 * 0.01]) for c in cands)

    class Cubic(position_profiles.PosProf):
        def step(self, t):
            return np.array([t, t ** 3, t])

    class Instant(velocity_profiles.VelProf):
        def generate(self, start_velocity, target_velocity):
            return np.array([start_velocity, target_velocity], dtype=float)

    table, off, cands = profile_tables(Cubic(n_sample_points=7), Instant(0.01), 0.3)
    assert len(cands) == 3 and np.array_equal(table[off[0]:off[0] + 21].reshape(7, 3)[:, 1], np.linspace(0, 1, 7) ** 3)


def test_orientation_matches_the_reference():
    _, data = path_cases.golden()
    q0, q1 = data["orientation_q0"], data["orientation_q1"]
    for fmt in ("euler", "quaternion"):
        o = Orientation(n_timesteps=50, output_format=fmt)
        got = o.generate_path(q0, q1)
        ref = data[f"orientation_{fmt}"]
        # the same libm formulas on both sides; operation order differs by a few roundings
        assert got.shape == ref.shape and np.abs(got - ref).max() < 1e-12
        assert np.array_equal(o.next(), got[0]) and np.array_equal(o.next(), got[1])
    with pytest.raises(ValueError, match="quaternion is required"):
        Orientation(n_timesteps=5).generate_path([0, 0, 0], q1)
    with pytest.raises(NotImplementedError):
        Orientation(n_timesteps=5).generate_path(q0, q1, dr=0.1)
    # match_position_path: fractions follow the position path (orientation.py:176-196)
    line = np.linspace(0, 1, 5)[:, None] ** 2 * np.ones(3)
    o = Orientation(output_format="quaternion")
    got = o.match_position_path(q0, q1, line)
    assert np.allclose(o.timesteps, np.linspace(0, 1, 5) ** 2) and np.allclose(got[0], q0) and np.allclose(got[-1], q1)
    assert _abi.euler_axes_code("rxyz") == 22 and _abi.euler_axes_code("sxyz") == 0
    assert len({_abi.euler_axes_code(a) for a in _abi.EULER_AXES}) == 24 and _abi.euler_axes_code((2, 1, 0, 1)) == 22
    with pytest.raises(ValueError):
        _abi.euler_axes_code("xyzr")


def test_path_params_layout_matches_header(tmp_path):
    src = r'''#include <stdio.h>
#include <stddef.h>
#include "abrk.h"
int main(){printf("%zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(abrk_path_params), offsetof(abrk_path_params, dt),
  offsetof(abrk_path_params, n_samples), offsetof(abrk_path_params, n_candidates), offsetof(abrk_path_params, axes),
  offsetof(abrk_path_params, width), offsetof(abrk_path_params, table_len), ABRK_EPATH);return 0;}'''
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-o", exe], input=src.encode(),
                   check=True)
    sizes = [int(v) for v in subprocess.run([exe], capture_output=True, check=True).stdout.split()]
    P = _abi.PathParams
    assert sizes == [C.sizeof(P), P.dt.offset, P.n_samples.offset, P.n_candidates.offset, P.axes.offset, P.width.offset,
                     P.table_len.offset, _abi.EPATH] == [32, 0, 8, 12, 16, 20, 24, -7]


def test_path_argument_validation_before_device():
    """every rejection of include/abrk.h's path planner section; none of them needs a device"""
    from abr_control_amd._lib import AbrkError, PathError, lib

    L = lib()
    for nm in ("abrk_path_plan_batch", "abrk_path_fill_batch", "abrk_path_next_batch"):
        assert hasattr(L, nm)
    assert L.abrk_version() == 100
    assert issubclass(PathError, ValueError) and issubclass(PathError, AbrkError)
    pos, vel = path_cases.profiles("case4")
    table, off, cands = profile_tables(pos, vel, 1.0)
    B, S, K = 3, pos.n_sample_points, len(cands)
    start, target = np.zeros((B, 3)), np.ones((B, 3))
    nt, rowplan, ds = np.zeros(B, np.int32), np.zeros((B, 2), np.int32), np.zeros((B, S))
    path = np.zeros((B, 4, 12))
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def plan(P, off_=off, B_=B, start_=start, table_=table):
        return L.abrk_path_plan_batch(C.byref(P) if P is not None else None, vp(table_), vp(off_), B_, vp(start_),
                                      vp(target), vp(nt), vp(rowplan), vp(ds), 0, None)

    def fill(P, off_=off, B_=B, t_max=4, so=start, path_=path):
        return L.abrk_path_fill_batch(C.byref(P), vp(table), vp(off_), B_, t_max, vp(start), vp(target), vp(so),
                                      vp(start), vp(nt), vp(rowplan), vp(ds), vp(path_), 0, None)

    def params(**kw):
        d = dict(dt=vel.dt, n_samples=S, n_candidates=K, axes=22, width=12, table_len=table.size)
        d.update(kw)
        return _abi.PathParams(*[d[f] for f, _ in _abi.PathParams._fields_])

    EINVAL = -1
    bad = [params(n_samples=1), params(n_samples=0), params(n_candidates=0), params(width=7), params(axes=3),
           params(axes=32), params(axes=-1), params(table_len=-1)]
    bad += [params(dt=v) for v in (0.0, -1e-3, np.inf, -np.inf, np.nan)]
    bad += [params(table_len=table.size - 1)]  # the last ramp now leaves the table
    for P in bad:
        assert plan(P) == EINVAL and fill(P) == EINVAL
        assert b"EINVAL" not in L.abrk_last_error() and L.abrk_last_error()
    ok = params()
    assert plan(ok, B_=-1) == EINVAL and fill(ok, B_=-1) == EINVAL
    assert plan(None) == EINVAL and plan(ok, start_=None) == EINVAL and plan(ok, table_=None) == EINVAL
    assert plan(ok, off_=None) == EINVAL
    for i, v in ((0, -1), (0, table.size), (1, table.size - 1), (2, -5), (3, table.size + 1), (5, 1 << 40),
                 (2 + 4 * (K - 1) + 2, table.size + 1)):
        o = off.copy()
        o[i] = v
        assert plan(ok, off_=o) == EINVAL and fill(ok, off_=o) == EINVAL, (i, v)
    assert fill(ok, t_max=0) == EINVAL and fill(ok, so=None) == EINVAL and fill(ok, path_=None) == EINVAL
    # an empty batch is a no-op even without a device
    assert plan(ok, B_=0) == 0 and fill(ok, B_=0) == 0

    counter, tgt = np.zeros(B, np.int32), np.zeros((B, 6))
    nxt = lambda dtype=0, B_=B, t_max=4, width=12, path_=path, counter_=counter, tgt_=tgt: L.abrk_path_next_batch(
        dtype, B_, t_max, width, vp(path_), vp(nt), vp(counter_), vp(tgt_), None, 0, None)
    assert nxt(dtype=7) == EINVAL and nxt(B_=-1) == EINVAL and nxt(t_max=0) == EINVAL and nxt(width=9) == EINVAL
    assert nxt(path_=None) == EINVAL and nxt(counter_=None) == EINVAL and nxt(tgt_=None) == EINVAL
    assert nxt(B_=0) == 0
    # the Python layer checks shapes and dtypes itself
    from abr_control_amd import engine

    with pytest.raises(ValueError):
        engine.path_plan(ok, table, off[:-1], start, target)
    with pytest.raises(ValueError):
        engine.path_plan(ok, table[:-1], off, start, target)
    with pytest.raises(ValueError):
        engine.path_next(path, nt.astype(np.int64), counter, tgt)
    with pytest.raises(ValueError):
        engine.path_next(path, nt, counter, tgt.astype(np.float32))  # target of another dtype than the call's
    with pytest.raises(AbrkError, match="EINVAL"):
        engine.path_plan(params(n_samples=1), table, off, start, target)


def test_path_planner_fails_loudly_without_gpu():
    from abr_control_amd import AbrkError, device_count

    if device_count() > 0:
        pytest.skip("a GPU is present")
    pos, vel = path_cases.profiles("case1")
    with pytest.raises(AbrkError, match="no HIP device"):
        PathPlanner(pos, vel).generate_path(np.zeros(3), np.ones(3) * 0.3, 1.0)
