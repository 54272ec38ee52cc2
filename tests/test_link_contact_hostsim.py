"""The row program of the whole-arm contact (abrk_link_contact.h link_contact_body) built for the host
(tests/hostsim_link_contact) against the NumPy reference (tests/link_contact_ref.py): tau and every report column for 130
rows of onejoint (one segment, joint0 -> EE), twojoint, threejoint, ur5, jaco2, ur5 as a runtime table and the
non-orthogonal synthetic4, both dtypes, one and eight obstacles per row.  Rows without force give tau exactly zero;
accumulate leaves them untouched to the bit; a switched-off segment, a zero-length segment and d == 0 behave as
include/abrk.h states.
Bars: 1e-6 (fp64) and 1e-4 (fp32) on max|d| / max|ref| per row for tau and the force; the integer columns exact.  Which
rows count, and why none is left out with these seeds: tests/link_contact_ref.py."""
import numpy as np
import pytest

from abr_control_amd import _abi
from tests import hostsim_link_contact as hl
from tests.link_contact_ref import CLEAR, IN, LEAVE, T0, T1, TWO, VS, LinkContactRef, check, draw_case, rel_err, tol_of

B = 130
SEED = 73
ARMS = ("onejoint", "twojoint", "threejoint", "ur5", "jaco2", "ur5_rt", "synthetic4")
DTYPES = pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))


def table_of(name):
    """-> (table, runtime)"""
    if name == "synthetic4":
        from tests import compiled_arms

        return _abi.normalize_table(compiled_arms.test_arms()["synthetic4"]), False
    return _abi.load_table("ur5" if name == "ur5_rt" else name), name == "ur5_rt"


def run(tab, rt, case, dtype, **kw):
    return hl.link_contact_step(tab, case["q"], case["dq"], case["obstacle"], case["radius"], VS, dtype=dtype,
                                runtime=rt, **kw)


@DTYPES
@pytest.mark.parametrize("K", (1, 8))
@pytest.mark.parametrize("name", ARMS)
def test_link_contact_hostsim_matches_the_reference(name, K, dtype):
    tab, rt = table_of(name)
    case = draw_case(tab, name, K, B, dtype, SEED)
    tau, rep = run(tab, rt, case, dtype)
    check(case, tau, rep, dtype, f"{name} K={K} {np.dtype(dtype).name}")


@pytest.mark.parametrize("name", ARMS)
def test_link_contact_reference_populates_every_branch(name):
    """on the reference alone: the cap on rows left out (none in fp64, at most one in fp32 - draw_case asserts it) and
    a population of every branch"""
    tab, _ = table_of(name)
    n = int(tab["n_joints"])
    for dtype in (np.float64, np.float32):
        for K in (1, 8):
            case = draw_case(tab, name, K, B, dtype, SEED)
            kind, rep = case["kind"], case["report"]
            assert (~case["keep"]).sum() <= (0 if dtype == np.float64 else 1)
            on = case["pushing"]
            assert (on & (kind == IN)).sum() >= B // 12 and (on & (kind == T0)).sum() >= B // 12
            assert (on & (kind == T1)).sum() >= B // 12
            assert (kind == CLEAR).sum() >= B // 12 and (rep[kind == CLEAR, 3] < 0).all()
            leave = (rep[:, 4] > 0) & ~on
            assert leave.sum() >= B // 12 and np.array_equal(leave, kind == LEAVE)
            if n >= 2:
                assert (kind == TWO).sum() >= B // 12 and (rep[kind == TWO, 4] >= 2).all()


@DTYPES
@pytest.mark.parametrize("name", ("ur5", "jaco2", "ur5_rt"))
def test_link_contact_hostsim_accumulate_adds_to_a_prefilled_array(name, dtype):
    tab, rt = table_of(name)
    n = int(tab["n_joints"])
    case = draw_case(tab, name, 8, B, dtype, SEED)
    pre = np.random.RandomState(7).uniform(-5, 5, (B, n)).astype(dtype)
    pre[1, 0] = -0.0  # (a clear row: + 0 would make it +0)
    tau, _ = run(tab, rt, case, dtype, tau=pre)
    on = case["pushing"] & case["keep"]
    assert not case["pushing"][1]
    assert tau[~case["pushing"]].tobytes() == pre[~case["pushing"]].tobytes()  # untouched to the bit
    want = pre.astype(np.float64) + case["tau"]
    e = rel_err(tau[on], want[on])
    print(f"{name} {np.dtype(dtype).name} accumulate {e:.2e}")
    assert e <= tol_of(dtype)
    assert rel_err(tau[on], pre[on]) > 1e-3  # the contact matters


@DTYPES
@pytest.mark.parametrize("name", ("ur5", "jaco2", "ur5_rt", "synthetic4"))
def test_link_contact_hostsim_a_switched_off_segment_takes_no_force(name, dtype):
    """only segment 1 on: tau past joint 1 is exactly zero, the report names segment 1 alone, and the case matches the
    reference drawn with the other segments off"""
    tab, rt = table_of(name)
    n = int(tab["n_joints"])
    case = draw_case(tab, name, 8, B, dtype, SEED, off=[i for i in range(n) if i != 1])
    tau, rep = run(tab, rt, case, dtype)
    check(case, tau, rep, dtype, f"{name} segment 1 only {np.dtype(dtype).name}")
    assert not tau[:, 2:].any() and np.abs(tau[case["pushing"], :2]).max() > 0
    assert (rep[:, 5] == 1).all()


def test_link_contact_hostsim_a_zero_length_segment_is_skipped():
    """twojoint with the EE moved onto the origin of joint 1, so that its second segment has zero length: an obstacle
    around that point pushes segment 0 alone - one pair counted, at t = 1 - and with segment 0 off no pair is active at
    all: tau = 0, no force, count 0, depth the lowest finite value, indices -1"""
    import copy

    tab = copy.deepcopy(_abi.load_table("twojoint"))
    for key in ("B", "E"):
        blk = tab[key][1] if key == "B" else tab[key]
        for r in range(3):
            blk[r][3] = 0.0
    q, dq = np.array([[0.3, -0.4]]), np.array([[0.5, 1.0]])
    ref = LinkContactRef(tab, [0.03, 0.03])
    a, b = ref.segments(q[0])
    assert np.array_equal(a[1], b[1]) and np.linalg.norm(b[0] - a[0]) > 0.1
    obs = np.array([[[*(a[1] + [0, 0.05, 0]), 0.05, 2e4, 20.0, 0.3]]])
    want_tau, want_rep, _, _ = ref.step(q, dq, obs)
    tau, rep = hl.link_contact_step(tab, q, dq, obs, [0.03, 0.03], VS)
    assert want_rep[0, 4] == 1 and np.array_equal(rep[0, 4:], [1, 0, 0, 1.0])
    assert rel_err(tau, want_tau) <= 1e-9 and rel_err(rep[:, :4], want_rep[:, :4]) <= 1e-9
    tau, rep = hl.link_contact_step(tab, q, dq, obs, [-1.0, 0.03], VS)
    assert not tau.any() and not rep[0, :3].any() and rep[0, 4] == 0
    assert rep[0, 3] == np.finfo(np.float64).min and rep[0, 5] == -1 and rep[0, 6] == -1


@DTYPES
@pytest.mark.parametrize("name", ("twojoint", "ur5"))
def test_link_contact_hostsim_a_centre_on_the_axis_counts_without_force(name, dtype):
    """d == 0: the obstacle's centre at the origin of joint 0, a constant of the table that the first segment starts
    from (t = 0, x = a to the bit): the pair is counted with delta = R + r, n = 0 gives no force, tau = 0 - and nothing
    is NaN"""
    tab, _ = table_of(name)
    n = int(tab["n_joints"])
    q, dq = np.full((1, n), 0.4), np.full((1, n), 0.7)
    radius = np.array([0.04] + [-1.0] * (n - 1))
    a, b = LinkContactRef(tab, radius).segments(q[0])
    c = a[0].astype(dtype).astype(np.float64)  # (the row program holds the constant rounded to its type as well)
    tau, rep = hl.link_contact_step(tab, q, dq, np.array([[[*c, 0.05, 1e4, 10.0, 0.2]]]), radius, VS, dtype=dtype)
    assert np.isfinite(tau).all() and np.isfinite(rep).all()
    assert abs(rep[0, 3] - 0.09) <= (1e-15 if dtype == np.float64 else 1e-8)
    assert np.array_equal(rep[0, 4:], [1, 0, 0, 0.0]) and not rep[0, :3].any() and not tau.any()
