"""The path planner's row programs (csrc/abrk_path.h, built for the host by tests/hostsim_path) against the reference's
own PathPlanner on every fixture case: step counts exact on every row, all columns within tests/path_cases.BOUND;
the orientation columns of all 24 Euler sequences against rotations composed in NumPy (no reference involved); rows
without a path, a movement exactly towards -(1,1,1)/sqrt(3) among them; a t_max below a row's step count.
Maxima observed here (max |difference| over all rows; printed by each run, recorded in DESIGN.md "Path planner")."""
import numpy as np
import pytest

from abr_control_amd import _abi
from abr_control_amd.controllers.path_planners import position_profiles, velocity_profiles
from abr_control_amd.controllers.path_planners.path_planner import profile_tables
from tests import hostsim_path, path_cases


@pytest.mark.parametrize("name", path_cases.names())
def test_hostsim_rows_match_the_reference(name):
    r = path_cases.rows(name)
    pos, vel = path_cases.profiles(name)
    path, nt = hostsim_path.generate_path(pos, vel, r["start"], r["target"], start_orientation=r["so"],
                                          target_orientation=r["to"], axes=r["axes"], **r["kwargs"])
    assert path.shape == (len(r["nt"]), r["nt"].max(), 6 if r["so"] is None else 12)
    path_cases.check_against_reference(name, path, nt, lambda what, v: print(f"hostsim {what}: {v:.3e}"))


def test_hostsim_rows_without_a_path():
    """start == target, and a movement too short for any candidate: n_timesteps 0, the other rows unaffected"""
    r = path_cases.rows("case4")
    pos, vel = path_cases.profiles("case4")
    start, target = r["start"].copy(), r["target"].copy()
    target[1] = start[1]
    target[3] = start[3] + 1e-7
    path, nt = hostsim_path.generate_path(pos, vel, start, target, start_orientation=r["so"], target_orientation=r["to"],
                                          **r["kwargs"])
    assert nt[1] == 0 and nt[3] == 0 and not path[1].any() and not path[3].any()
    keep = [0, 2, 4, 5]
    assert np.array_equal(nt[keep], r["nt"][keep])
    for b in keep:
        assert np.abs(path[b, :nt[b]] - r["paths"][b]).max() < path_cases.BOUND


@pytest.mark.parametrize("axes", sorted(_abi.EULER_AXES))
def test_hostsim_orientation_columns_lie_on_the_geodesic(axes):
    start, target, so, to = path_cases.geodesic_rows(axes)
    vel = velocity_profiles.Gaussian(dt=path_cases.GEODESIC_DT, acceleration=4)
    path, nt = hostsim_path.generate_path(position_profiles.Linear(), vel, start, target, 1.0, so, to, axes=axes)
    assert nt.min() >= 2
    path_cases.check_geodesic(axes, path, nt, so, to, lambda line: print("hostsim", line))


def test_hostsim_no_path_exactly_towards_the_antidiagonal():
    """target = start - 0.25 (1,1,1)/sqrt(3): align_vectors divides by 1 + cs = 0 there and the reference raises.  In a
    batch of four that row has n_timesteps 0 and stays zero; the other three equal their own single-row runs.
    (Before path_row_setup tested 1 + cs this row came back with n_timesteps 124 and NaN in every column.)"""
    pos, vel = position_profiles.Linear(), velocity_profiles.Gaussian(dt=0.004, acceleration=4)
    start, target, so, to = path_cases.antidiagonal_batch()
    path, nt = hostsim_path.generate_path(pos, vel, start, target, 1.0, so, to)
    assert nt[2] == 0 and not path[2].any(), (nt, path[2, 0])
    assert np.isfinite(path).all()
    for b in (0, 1, 3):
        one, n1 = hostsim_path.generate_path(pos, vel, start[b:b + 1], target[b:b + 1], 1.0, so[b:b + 1], to[b:b + 1])
        assert nt[b] == n1[0] >= 2 and np.array_equal(path[b, :nt[b]], one[0])


def test_hostsim_t_max_below_a_rows_step_count():
    """path_fill with t_max = max(n_timesteps) - 1 on the rows of case1: a row that does not fit keeps what the array
    held in every column, the others equal the normal call's rows cut at t_max bit for bit"""
    r = path_cases.rows("case1")
    pos, vel = path_cases.profiles("case1")
    full, nt = hostsim_path.generate_path(pos, vel, r["start"], r["target"], start_orientation=r["so"],
                                          target_orientation=r["to"], **r["kwargs"])
    t_max = int(nt.max()) - 1
    cut = hostsim_path.fill(pos, vel, r["start"], r["target"], r["so"], r["to"], t_max, sentinel=-7.0, **r["kwargs"])
    path_cases.check_truncated_fill(cut, full, nt, t_max, -7.0)
