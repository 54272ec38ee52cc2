"""The path planner's row programs (csrc/abrk_path.h, built for the host by tests/hostsim_path) against the reference's
own PathPlanner on every fixture case: step counts exact on every row, all columns within tests/path_cases.BOUND.
Maxima observed here (max |difference| over all rows; printed by each run, recorded in DESIGN.md "Path planner")."""
import numpy as np
import pytest

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
