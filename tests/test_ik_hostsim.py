"""The inverse-kinematics row program (csrc/abrk_ctrl.h ik_row, pinv_KxN, quat_from_R) in its host build against the
C oracle, one step at a time: float64 and float32, the three methods, arms of 1 - 7 joints as built-in and as table
arms.  Cases, gates, the cap on what is left out and the bar: tests/ik_cases.py; figures: profiles/ik_tests.md.
Run with -s to see, per case, the share of pairs left out, the worst error / bar and the sides of the clamps."""
import numpy as np
import pytest

from tests import ik_cases as K

ARMS = ["onejoint", "twojoint", "threejoint", "ur5", "jaco2", "synth1", "synth4", "synth5", "synth7", "ur5_rt"]
BUILTIN = ("onejoint", "twojoint", "threejoint", "ur5", "jaco2")


def _run(arm_id, dtype):
    from tests import hostsim

    arm = arm_id if arm_id in BUILTIN else K.arm_table(arm_id)
    return lambda p, q, tgt: hostsim.ik_generate_path(arm, p, q, tgt, dtype=dtype)


@pytest.mark.parametrize("method", (1, 2, 3))
@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("arm_id", ARMS)
def test_rows_ik_steps_against_oracle(arm_id, dtype, method):
    """B = 64, T = 1 at random postures (with the singular block and the near-target rows) under the three limit sets,
    then B = 16, T = 40 teacher-forced from a reachable draw under the default and the wide limits; every clamp seen
    engaged and not engaged on the reference"""
    run, clamps = _run(arm_id, dtype), K.Clamps()
    K.run_one_step(run, arm_id, dtype, method, 64, K.SEED_STEP, clamps)
    for limits in ("default", "wide"):
        K.run_path(run, arm_id, dtype, method, 16, 40, K.SEED_PATH, limits, clamps, free_running=limits == "default")
    clamps.check(f"{arm_id} method {method}")
    print(f"{arm_id} method {method}: every clamp seen engaged and not engaged")


@pytest.mark.parametrize("method", (1, 2, 3))
@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
def test_numpy_in_dtype_needs_a_quarter_of_the_bar(dtype, method):
    """the bar's constant: the three formulas in plain NumPy in the dtype, from the oracle's J, dx and dr rounded to it,
    stay within C / 4 on every counted pair of the cases above (profiles/ik_tests.md holds the figures)"""
    dt, worst, issue = np.dtype(dtype), 0.0, 0.0
    for arm_id in ARMS:
        q, tgt, block, refs = K.one_step_case(arm_id, 64, K.SEED_STEP, dt.name, method)
        refs = list(refs.values()) + [K.path_case(arm_id, 16, 40, K.SEED_PATH, dt.name, method, lim)[4] for lim in ("default", "wide")]
        for i, r in enumerate(refs):
            ok = K.counted(r, dt) & ((block != 0) if (dt == K.F32 and i < 3) else True)
            worst = max(worst, K.numpy_needs(r, dt)[ok].max(initial=0.0))
            issue = max(issue, np.nan_to_num(K.numpy_needs(r, dt, issue_formula=True)[ok], nan=0.0).max(initial=0.0))
    print(f"NumPy in {dt.name}, method {method}: needs {worst:.3g} of C = {K.C:g}; without the residual and forward-"
          f"kinematics terms of the bar (C eps kappa scale alone) it would need {issue:.3g}")
    assert worst <= K.C / 4


@pytest.mark.parametrize("arm_id", ("synth3",))
def test_rows_ik_next_to_a_singularity_float32(arm_id):
    """32 postures with kappa of 200 - 700: they count in float32 and lie far beyond the gate of pinv_KxN's Cholesky path
    (trace^3 < 1e2 det), which at that kappa would lose eps kappa^2, more than the bar; the Jacobi fallback keeps it"""
    K.run_ill(_run(arm_id, np.float32), arm_id, np.float32, 32, 6)
