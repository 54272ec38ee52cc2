"""The row program of the end-effector contact (abrk_contact.h contact_body) built for the host (tests/hostsim_contact)
against the NumPy reference (tests/contact_ref.py): tau and the report for 130 rows of twojoint, threejoint, ur5, jaco2
and ur5 as a runtime table, both dtypes, one and three surfaces per row; the tip at the EE with and without a tool
offset and on a mid-chain frame (link2; joint1 on the two-joint arm), whose torques past the frame are exact zeros.
Rows without force give tau exactly zero; accumulate adds to a pre-filled array.
Bars: 1e-6 (fp64) and 1e-4 (fp32) on max|d| / max|ref| per row for tau and the report's two force triples.  Which rows
count, and why none is left out with these seeds: tests/contact_ref.py."""
import numpy as np
import pytest

from abr_control_amd import _abi
from tests import hostsim_contact as hc
from tests.contact_ref import VS, check, draw_case, rel_err, tol_of

B = 130
SEED = 61
ARMS = ("twojoint", "threejoint", "ur5", "jaco2", "ur5_rt")
OFFSET = (0.03, -0.02, 0.11)


def table_of(name):
    return _abi.load_table("ur5" if name == "ur5_rt" else name), name == "ur5_rt"


def mid_frame(n):
    return "joint1" if n == 2 else "link2"


def frames(n):
    """(frame, offset) of the issue's cases; the mid-chain point carries an offset as well, so that it moves"""
    return (("EE", (0, 0, 0)), ("EE", OFFSET), (mid_frame(n), OFFSET))


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("S", (1, 3))
@pytest.mark.parametrize("which", (0, 1, 2), ids=("EE", "EE_offset", "mid"))
@pytest.mark.parametrize("name", ARMS)
def test_contact_hostsim_matches_the_reference(name, which, S, dtype):
    tab, rt = table_of(name)
    n = int(tab["n_joints"])
    frame, off = frames(n)[which]
    case = draw_case(tab, name, frame, off, S, B, dtype, SEED)
    tau, rep = hc.contact_step(tab, case["q"], case["dq"], case["surface"], frame, off, VS, dtype=dtype, runtime=rt)
    check(case, tau, rep, dtype, f"{name} {frame} {off} S={S} {np.dtype(dtype).name}")
    if which == 2:
        m = _abi.frame_id(frame, n) // 2  # the joints the frame hangs off
        assert 0 < m < n
        assert not tau[:, m:].any(), "a joint past the frame takes torque"
        assert np.abs(tau[case["pressing"], :m]).max() > 0


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("ur5", "jaco2", "ur5_rt"))
def test_contact_hostsim_accumulate_adds_to_a_prefilled_array(name, dtype):
    tab, rt = table_of(name)
    n = int(tab["n_joints"])
    case = draw_case(tab, name, "EE", OFFSET, 3, B, dtype, SEED)
    pre = np.random.RandomState(7).uniform(-5, 5, (B, n)).astype(dtype)
    tau, _ = hc.contact_step(tab, case["q"], case["dq"], case["surface"], "EE", OFFSET, VS, tau=pre, dtype=dtype,
                             runtime=rt)
    on = case["pressing"] & case["keep"]
    assert np.array_equal(tau[~case["pressing"]], pre[~case["pressing"]])  # + 0 exactly
    want = pre.astype(np.float64) + case["tau"]
    e = rel_err(tau[on], want[on])
    print(f"{name} {np.dtype(dtype).name} accumulate {e:.2e}")
    assert e <= tol_of(dtype)
    assert rel_err(tau[on], pre[on]) > 1e-2  # the contact matters


def test_contact_hostsim_a_normal_is_used_as_given_and_friction_opposes_sliding():
    """one UR5 row 20 mm into a horizontal floor: the friction part of F points against the tangential velocity with
    |Ft| <= mu fn; and with n = (0, 0, 2), d chosen for the same delta, the law is evaluated on that n as it stands - vn
    and the direction fn n both double (no normalisation inside the row program)"""
    tab, _ = table_of("ur5")
    case = draw_case(tab, "ur5", "EE", (0, 0, 0), 1, B, np.float64, SEED)
    q, dq, ref = case["q"][:1], case["dq"][:1], case["ref"]
    p, Jp = ref.point(q[0])
    v = Jp @ dq[0]
    k, c, mu = 2e4, 20.0, 0.5
    s = np.array([[[0, 0, 1.0, p[2] + 0.02, k, c, mu, 0.0]]])
    _, rep = hc.contact_step(tab, q, dq, s, vs=VS)
    F = rep[0, :3]
    assert F[2] > 0 and abs(rep[0, 6] - 0.02) < 1e-12 and rep[0, 7] == 1
    assert abs(F[2] - (k * 0.02 - c * v[2])) <= 1e-9 * F[2]
    assert F[:2] @ v[:2] < 0 and np.linalg.norm(F[:2]) <= mu * F[2] * (1 + 1e-12)
    s2 = s.copy()
    s2[0, 0, :4] = [0, 0, 2.0, 2 * p[2] + 0.02]
    tau2, rep2 = hc.contact_step(tab, q, dq, s2, vs=VS)
    want_tau, want_rep, _ = ref.step(q, dq, s2)
    assert abs(rep2[0, 6] - 0.02) < 1e-12 and rel_err(rep2[:, :3], rep[:, :3]) > 0.1  # (normalised, it would be F)
    assert rel_err(rep2[:, :3], want_rep[:, :3]) <= 1e-12 and rel_err(tau2, want_tau) <= 1e-12
