"""General-inertia arms on the GPU (compiled plugins of tests/compiled_inertia_arms.py): dynamics, the fused OSC laws and
the controllers against the reference's own outputs (tests/golden/inertia_<arm>.npz, tools/gen_inertia_golden.py)."""
import numpy as np
import pytest

from abr_control_amd import _abi, engine
from tests import compiled_inertia_arms
from tests.cases import TOL_D
from tests.test_general_inertia import fixture

pytestmark = pytest.mark.gpu
ARMS = compiled_inertia_arms.ARMS
XYZ, SIX = [True, True, True, False, False, False], [True] * 6


@pytest.fixture(scope="module")
def configs():
    from abr_control_amd import arms

    out = {arm: arms.from_table(fixture(arm)[0]) for arm in ARMS}
    for rc in out.values():
        assert rc.plugin_path is not None
    yield out
    for rc in out.values():
        rc.close()


def _rel(a, b):
    return np.max(np.abs(np.asarray(a, float) - b)) / np.max(np.abs(b))


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dynamics_match_the_reference(configs, arm, dtype):
    tab, z = fixture(arm)
    rc = configs[arm]
    q, dq = z["dyn_q"], z["dyn_dq"]
    want = ("M", "g", "C") if "C" in z.files else ("M", "g")
    res = engine.dynamics(rc.arm_id, rc.N_JOINTS, q.astype(dtype), dq.astype(dtype), None, None, want, dtype)
    tol = 1e-10 if dtype == np.float64 else 1e-4
    for k in want:
        assert _rel(res[k], z[k]) < tol, f"{arm} {k} {np.dtype(dtype).name}: {_rel(res[k], z[k]):.2e}"
    for f in z["frames"]:  # kinematics are unaffected
        J = engine.dynamics(rc.arm_id, rc.N_JOINTS, q, None, rc.frame_id(str(f)), None, ("J",))["J"]
        assert _rel(J, z[f"J_{f}"]) < 1e-10 if np.any(z[f"J_{f}"]) else not np.any(J)


@pytest.mark.parametrize("arm", ARMS)
def test_inertia_is_symmetric_positive_definite_and_mdot_minus_2c_is_skew(configs, arm):
    rc = configs[arm]
    n = rc.N_JOINTS
    rng = np.random.RandomState(3)
    q, dq = rng.uniform(0, 2 * np.pi, (64, n)), rng.uniform(-3, 3, (64, n))
    d = engine.dynamics(rc.arm_id, n, q, dq, None, None, ("M", "C"))
    M, Cm = d["M"], d["C"]
    assert np.array_equal(M, np.swapaxes(M, 1, 2))
    assert np.all(np.linalg.eigvalsh(M) > 0)
    h = 1e-5  # Mdot along dq, central difference
    Mp = engine.dynamics(rc.arm_id, n, q + h * dq, None, None, None, ("M",))["M"]
    Mm = engine.dynamics(rc.arm_id, n, q - h * dq, None, None, None, ("M",))["M"]
    S = (Mp - Mm) / (2 * h) - 2 * Cm
    assert np.max(np.abs(S + np.swapaxes(S, 1, 2))) / np.max(np.abs(Cm)) < 1e-6


def test_ur5_rotor_inertias_add_exactly_their_joint_terms(configs):
    """M_GI - M_plain = sum_j J_joint_j^T mjoint_j J_joint_j, with the package's own (pinned) J('joint j')"""
    from abr_control_amd.arms import ur5

    tab, z = fixture("ur5")
    plain = ur5.Config()
    q = z["dyn_q"]
    Mg = engine.dynamics(configs["ur5"].arm_id, 6, q, None, None, None, ("M",))["M"]
    Mp = engine.dynamics(plain.arm_id, 6, q, None, None, None, ("M",))["M"]
    want = np.zeros_like(Mg)
    for j in range(6):
        J = engine.dynamics(plain.arm_id, 6, q, None, plain.frame_id(f"joint{j}"), None, ("J",))["J"]
        want += np.einsum("bri,rs,bsj->bij", J, np.array(tab["mjoint"][j]), J)
    assert np.max(np.abs(want)) > 1e-3  # the rotors matter
    assert np.max(np.abs((Mg - Mp) - want)) / np.max(np.abs(Mg)) < 1e-12


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("rows", [4096, 300_032])
def test_fused_osc_equals_the_law_on_the_reference_dynamics(configs, arm, rows):
    """every fused OSC kernel (x,y,z and six task rows, use_C on / off, with and without training signal) equals
    abrk_osc_law_batch fed the reference's fp64 J, M, g, C dq (kinematics Tx / R from the package)"""
    tab, z = fixture(arm)
    rc = configs[arm]
    n = rc.N_JOINTS
    idx = np.arange(rows) % z["dyn_q"].shape[0]
    q, dq = z["dyn_q"][idx], z["dyn_dq"][idx]
    tgt = np.random.RandomState(rows).uniform(-1, 1, (rows, 6))
    J, M, g = z["J_EE"][idx], z["M"][idx], z["g"][idx]
    kin = engine.dynamics(rc.arm_id, n, q, None, None, None, ("Tx", "R"))
    for use_C in ((False, True) if "C" in z.files else (False,)):
        Cdq = np.einsum("bij,bj->bi", z["C"][idx], dq) if use_C else None
        for dof, kw in ((XYZ, dict(kp=200)), (SIX, dict(kp=200, ko=150, kv=25))):
            P = _abi.make_osc_params(n, ctrlr_dof=dof, use_C=use_C, **kw)
            # the fused "u + robot_config outputs" kernel hands out the same M, g (and C) it used
            _, outs = engine.osc_generate(rc.arm_id, n, P, q, dq, tgt, want=("M", "g", "C") if use_C else ("M", "g"))
            assert _rel(outs["M"], M) < 1e-10 and _rel(outs["g"], g) < 1e-10
            if use_C:
                assert _rel(outs["C"], z["C"][idx]) < 1e-10
            for ts in (False, True):
                got = engine.osc_generate(rc.arm_id, n, P, q, dq, tgt, training_signal=ts)
                ref = engine.osc_law(n, P, J, M, dq, tgt, g=g, Cdq=Cdq, xyz=kin["Tx"], R=kin["R"], q=q,
                                     training_signal=ts)
                for a, b in zip(got if ts else (got,), ref if ts else (ref,)):
                    err = np.max(np.abs(a - b), axis=1) / np.maximum(np.max(np.abs(b), axis=1), 1e-300)
                    assert err.max() < 1e-9, f"{arm} dof={sum(dof)} C={use_C} ts={ts}: {err.max():.2e}"


@pytest.mark.parametrize("arm", ARMS)
def test_controllers_match_the_reference(configs, arm):
    """OSC, Sliding, Joint, Floating on a general-inertia robot_config, against the reference's controllers on the same
    config (fp64 formulas); tolerance of the existing secondary-controller tests"""
    from abr_control_amd.controllers import OSC, Floating, Joint, Sliding

    tab, z = fixture(arm)
    rc = configs[arm]
    cases = {
        "joint": lambda q, dq, t: Joint(rc, kp=50, kv=9).generate(q, dq, t * 3.0),
        "floating": lambda q, dq, t: Floating(rc, dynamic=True).generate(q, dq),
        "osc_xyz": lambda q, dq, t: OSC(rc, kp=200, ctrlr_dof=XYZ).generate(q, dq, t),
        "osc6": lambda q, dq, t: OSC(rc, kp=200, ko=150, kv=25, ctrlr_dof=SIX).generate(q, dq, t),
    }
    if "C" in z.files:
        cases["sliding"] = lambda q, dq, t: Sliding(rc).generate(q, dq, t)
        cases["osc_xyz_C"] = lambda q, dq, t: OSC(rc, kp=200, ctrlr_dof=XYZ, use_C=True).generate(q, dq, t)
        cases["osc6_C"] = lambda q, dq, t: OSC(rc, kp=200, ko=150, kv=25, ctrlr_dof=SIX, use_C=True).generate(q, dq, t)
    for key, run in cases.items():
        ref = z[f"{key}_u"]
        u = np.asarray(run(z[f"{key}_q"], z[f"{key}_dq"], z[f"{key}_target"]), float)
        err = np.max(np.abs(u - ref), axis=1) / np.maximum(np.max(np.abs(ref), axis=1), 1e-9)
        assert err.max() <= TOL_D, f"{arm} {key}: {err.max():.3e}"
