"""The loop recorder's row program (abr_control_amd/csrc/abrk_trace.h) built for the host (tests/hostsim_trace) against
the oracle's Tx, the source arrays and NumPy statistics - no GPU needed.  Compile-time tables of UR5, Jaco2 and twojoint,
and UR5's table as a runtime-table arm; ref_frame "EE" and one link frame with an offset; fp64 and fp32."""
import numpy as np
import pytest

from abr_control_amd import _abi
from tests import trace_cases as tc

CASES = [(arm, False) for arm in tc.ARMS] + [("ur5", True)]


def _tick(table, runtime):
    from tests.hostsim_trace import HostTrace

    return HostTrace(table, runtime=runtime)


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("which", tc.FRAMES)
@pytest.mark.parametrize("arm,runtime", CASES, ids=[a + ("_rt" if r else "") for a, r in CASES])
def test_hostsim_loop_trace_parity(arm, runtime, which, dtype):
    table = _abi.load_table(arm)
    tc.check_case(_tick(table, runtime), table, arm, which, dtype)


def test_hostsim_history_only_and_stats_only_leave_the_other_alone():
    table = _abi.load_table("ur5")
    tick = _tick(table, False)
    n, src = 6, tc.inputs(6, 5)
    mask = _abi.trace_columns_mask(("xyz", "err"))
    fid = _abi.frame_id("EE", n)
    both = tc.run(tick, n, np.float64, src, mask, 1, tc.T_TICKS, 0.5, fid, None)
    h, st, se, c = tc.run(tick, n, np.float64, src, mask, 1, tc.T_TICKS, 0.5, fid, None, stats=False)
    assert st is None and np.array_equal(h, both[0]) and np.array_equal(c, both[3])
    h, st, se, c = tc.run(tick, n, np.float64, src, mask, 1, tc.T_TICKS, 0.5, fid, None, history=False)
    assert h is None and np.array_equal(st, both[1]) and np.array_equal(se, both[2])


def test_hostsim_restarted_rows_write_their_own_slots():
    """rows 1..2 restarted before tick 4, every=2: they write slots 0, 1 again while the others write slots 2, 3"""
    table = _abi.load_table("twojoint")
    tick = _tick(table, False)
    n, src = 2, tc.inputs(2, 5, T=8)
    mask = _abi.trace_columns_mask(("q", "err"))
    fid = _abi.frame_id("EE", n)
    h, st, se, c = tc.run(tick, n, np.float64, src, mask, 2, 4, 0.5, fid, None, resets=((4, 1, 3),))
    q = np.asarray(src[0])
    assert np.array_equal(c, [8, 4, 4, 8, 8])
    for b in (0, 3, 4):
        assert np.array_equal(h[:, b, :2], q[[0, 2, 4, 6], b])
    for b in (1, 2):
        assert np.array_equal(h[:2, b, :2], q[[4, 6], b]) and (h[2:, b] == tc.SENTINEL).all()
    errs = np.linalg.norm(np.asarray(src[3])[..., :3] - tc.oracle_tx(table, "EE", None, q), axis=-1)
    assert np.allclose(st[1:3, 1], errs[4:, 1:3].max(axis=0), rtol=1e-9)  # statistics of the second run alone
