"""C ABI and Python surface of the whole-arm contact (abrk_link_contact_step_batch, link_contact.link_contact_step,
obstacle_rows, Obstacles.from_controller's rows, ArmSim(obstacles=...)): the struct's layout, what bad params and a bad
host obstacle array are refused with - before any device use, naming row and obstacle - and what the Python layer passes
on.  No GPU needed."""
import ctypes as C
import re

import numpy as np
import pytest

from abr_control_amd import _abi, contact, link_contact


def _obstacle(B=5, K=2):
    s = np.zeros((B, K, 7))
    s[:, :, :] = [0.3, 0.1, 0.4, 0.05, 1e4, 100.0, 0.5]
    return s


def test_link_contact_struct_layout_and_export():
    import abr_control_amd
    from abr_control_amd._lib import lib

    P = _abi.LinkContactParams
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("n_obstacles", 0), ("link_radius", 8), ("vs", 64),
                                                                   ("accumulate", 72)]
    assert C.sizeof(P) == 80 and _abi.LINK_CONTACT_MAX_OBSTACLES == 8
    L = lib()
    assert L.abrk_version() == 100
    assert hasattr(L, "abrk_link_contact_step_batch") and len(L.abrk_link_contact_step_batch.argtypes) == 11
    p = _abi.make_link_contact_params(6)
    assert (p.n_obstacles, tuple(p.link_radius), p.vs, p.accumulate) == (1, (0.04,) * 6 + (-1.0,), 1e-3, 0)
    p = _abi.make_link_contact_params(3, 8, (0.02, -1, 0.05), 0.01, True)
    assert (p.n_obstacles, tuple(p.link_radius)[:4], p.vs, p.accumulate) == (8, (0.02, -1.0, 0.05, -1.0), 0.01, 1)
    with pytest.raises(ValueError, match="link_radius"):
        _abi.make_link_contact_params(6, link_radius=(0.1, 0.2))
    assert abr_control_amd.Obstacles is link_contact.Obstacles


def test_the_header_states_the_law():
    import os

    h = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "abrk.h")).read()
    assert "abrk_link_contact_step_batch" in h and "ABRK_LINK_CONTACT_MAX_OBSTACLES 8" in h
    assert "double link_radius[7]" in h


# (column, value, what the message names)
BAD = [
    (3, 0.0, r"R=0 is not > 0"),
    (3, -0.05, r"R=-0\.05 is not > 0"),
    (4, -1.0, r"k=-1"),
    (5, -0.5, r"c=-0\.5"),
    (6, -0.1, r"mu=-0\.1"),
    (1, np.nan, r"cy is not finite"),
    (3, np.inf, r"R is not finite"),
    (4, np.inf, r"k is not finite"),
    (6, -np.inf, r"mu is not finite"),
]


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("col,value,message", BAD, ids=[f"{i}" for i in range(len(BAD))])
def test_a_bad_host_obstacle_is_refused_before_the_device_naming_row_and_obstacle(col, value, message, dtype):
    from abr_control_amd import AbrkError

    q = np.zeros((5, 6), dtype)
    s = _obstacle().astype(dtype)
    s[3, 1, col] = value
    with pytest.raises(AbrkError, match="EINVAL") as ei:
        link_contact.link_contact_step(0, 6, _abi.make_link_contact_params(6, 2), q, q, s, None, dtype=dtype)
    msg = str(ei.value)
    assert re.search(message, msg) and "row 3, obstacle 1" in msg and "obstacle:" in msg, msg
    # the Python-side check of Obstacles / ArmSim says the same, naming the column too, before it copies anything
    with pytest.raises(ValueError, match=f"row 3, obstacle 1: {_abi.LINK_OBSTACLE[col]}"):
        link_contact.obstacle_rows(s, 5)


def test_zeros_of_either_sign_pass_the_validation():
    """zeros of either sign in k, c, mu: what refuses the call afterwards is the missing device"""
    from abr_control_amd import AbrkError, device_count

    q = np.zeros((2, 6))
    s = _obstacle(2, 1)
    s[1, 0, 4:] = [-0.0, 0.0, -0.0]
    link_contact.obstacle_rows(s, 2)
    p = _abi.make_link_contact_params(6)
    if device_count() > 0:
        tau, rep = link_contact.link_contact_step(0, 6, p, q, q, s, None, report=True)
        assert tau.shape == (2, 6) and rep.shape == (2, 8)
    else:
        with pytest.raises(AbrkError, match="ENODEV"):
            link_contact.link_contact_step(0, 6, p, q, q, s, None)


def test_bad_params_are_einval_before_the_device():
    from abr_control_amd import AbrkError, device_count
    from abr_control_amd._lib import lib

    q, s = np.zeros((2, 6)), _obstacle(2, 1)
    mk = _abi.make_link_contact_params
    step = link_contact.link_contact_step
    with pytest.raises(AbrkError, match="ENOARM"):
        step(999, 6, mk(6), q, q, s, None)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    L, tau = lib(), np.zeros((2, 6))
    for K in (0, 9, -1):
        p = mk(6)
        p.n_obstacles = K
        assert L.abrk_link_contact_step_batch(0, 0, C.byref(p), 2, vp(q), vp(q), vp(s), vp(tau), None, 0, None) == -1
        assert b"n_obstacles" in L.abrk_last_error()
    for vs in (0.0, -1e-3, np.inf, np.nan):
        with pytest.raises(AbrkError, match="EINVAL.*vs"):
            step(0, 6, mk(6, vs=vs), q, q, s, None)
    for bad in (np.nan, np.inf):
        with pytest.raises(AbrkError, match=r"EINVAL.*link_radius\[2\]"):
            step(0, 6, mk(6, link_radius=(0.04, 0.04, bad, 0.04, 0.04, 0.04)), q, q, s, None)
    with pytest.raises(AbrkError, match="EINVAL.*every segment"):
        step(0, 6, mk(6, link_radius=-1.0), q, q, s, None)
    # (radii past the arm's joints are not looked at: a three-joint arm with junk behind its three radii)
    p3 = mk(3)
    p3.link_radius[5] = np.nan
    q3 = np.zeros((2, 3))
    three = list(_abi.BUILTIN_ARMS).index("threejoint")
    rc = L.abrk_link_contact_step_batch(three, 0, C.byref(p3), 2, vp(q3), vp(q3), vp(s), vp(np.zeros((2, 3))), None, 0,
                                        None)
    assert rc == (0 if device_count() > 0 else -2), L.abrk_last_error()
    ok = mk(6)
    assert L.abrk_link_contact_step_batch(0, 0, None, 2, vp(q), vp(q), vp(s), vp(tau), None, 0, None) == -1
    assert L.abrk_link_contact_step_batch(0, 7, C.byref(ok), 2, vp(q), vp(q), vp(s), vp(tau), None, 0, None) == -1
    for hole in range(4):  # q, dq, obstacle and tau are required ...
        args = [vp(q), vp(q), vp(s), vp(tau)]
        args[hole] = None
        assert L.abrk_link_contact_step_batch(0, 0, C.byref(ok), 2, *args, None, 0, None) == -1
        assert b"required" in L.abrk_last_error()
    # ... a NULL report is accepted: with everything else in order the call goes on to the device (or its absence)
    rc = L.abrk_link_contact_step_batch(0, 0, C.byref(ok), 2, vp(q), vp(q), vp(s), vp(tau), None, 0, None)
    assert rc == (0 if device_count() > 0 else -2)  # ABRK_ENODEV
    # an empty batch is a no-op even without a device
    e = np.zeros((0, 6))
    assert step(0, 6, ok, e, e, np.zeros((0, 1, 7)), None).shape == (0, 6)
    # shape and dtype are caught in Python
    with pytest.raises(ValueError, match="obstacle"):
        step(0, 6, ok, q, q, np.zeros((2, 2, 7)), None)
    with pytest.raises(ValueError, match="accumulate"):
        step(0, 6, mk(6, accumulate=True), q, q, s, None)


class _Recorder:
    """stands in for the loaded library: records the entry point called and its arguments, returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0

        return call


def test_link_contact_step_passes_its_arrays_on(monkeypatch):
    fake = _Recorder()
    monkeypatch.setattr(link_contact, "lib", lambda: fake)
    q, s = np.zeros((3, 6)), _obstacle(3, 2)
    tau = np.ones((3, 6))
    mk = _abi.make_link_contact_params
    out = link_contact.link_contact_step(0, 6, mk(6, 2, accumulate=True), q, q, s, tau)
    name, a = fake.calls[-1]
    assert out is tau and name == "abrk_link_contact_step_batch" and len(a) == 11
    assert a[3] == 3 and a[6] == s.ctypes.data and a[7] == tau.ctypes.data and a[8] is None
    out, rep = link_contact.link_contact_step(0, 6, mk(6, 2), q, q, s, None, report=True)
    assert out.shape == (3, 6) and rep.shape == (3, 8) and fake.calls[-1][1][8] == rep.ctypes.data


def test_obstacle_rows_broadcasts_and_checks_shapes():
    one = _obstacle(1, 2)[0]
    p = link_contact.obstacle_rows(one, 4)
    assert p.shape == (4, 2, 7) and p.dtype == np.float64 and p.flags.c_contiguous and np.array_equal(p[3], one)
    assert link_contact.obstacle_rows(_obstacle(4, 8), 4).shape == (4, 8, 7)
    for bad in (np.zeros(7), np.zeros((2, 8)), _obstacle(3, 2), _obstacle(4, 9), np.zeros((0, 7))):
        with pytest.raises(ValueError, match="obstacles"):
            link_contact.obstacle_rows(bad, 4)
    d = link_contact.report_dict(np.arange(16.0).reshape(2, 8))
    assert np.array_equal(d["force"], [[0, 1, 2], [8, 9, 10]]) and np.array_equal(d["depth"], [3, 11])
    assert d["n_contacts"].tolist() == [4, 12] and d["segment"].tolist() == [5, 13]
    assert d["obstacle"].tolist() == [6, 14] and np.array_equal(d["t"], [7, 15])


def test_obstacles_from_controller_takes_the_avoided_spheres():
    """the rows Obstacles.from_controller builds, without a device: the controller's [x, y, z, r] with k, c, mu behind"""
    from abr_control_amd.arms import ur5
    from abr_control_amd.controllers import AvoidObstacles

    seen = {}

    class Probe(link_contact.Obstacles):
        def __init__(self, rc, B, obstacles, **kw):
            seen.update(rc=rc, B=B, rows=np.asarray(obstacles), kw=kw)

    rc = ur5.Config()
    avoid = AvoidObstacles(rc, obstacles=[[0.3, 0.1, 0.4, 0.05], [0.0, 0.5, 0.2, 0.1]])
    Probe.from_controller(avoid, 7, k=2e4, c=40.0, link_radius=0.03)
    assert seen["rc"] is rc and seen["B"] == 7 and seen["kw"] == {"link_radius": 0.03}
    assert np.array_equal(seen["rows"], [[0.3, 0.1, 0.4, 0.05, 2e4, 40.0, 0.0], [0.0, 0.5, 0.2, 0.1, 2e4, 40.0, 0.0]])
    assert link_contact.obstacle_rows(seen["rows"], 7).shape == (7, 2, 7)


def test_arm_sim_takes_obstacles(monkeypatch):
    from abr_control_amd import plant_payload
    from abr_control_amd.arms import ArmSim, ur5

    rc = ur5.Config()
    seen, planes, steps = [], [], []
    monkeypatch.setattr(plant_payload, "plant_step", lambda *a, **k: steps.append(k))
    monkeypatch.setattr(link_contact, "link_contact_step",
                        lambda *a, **k: seen.append((a, k)) or (np.full((1, 6), 2.0), np.zeros((1, 8))))
    monkeypatch.setattr(contact, "contact_step",
                        lambda *a, **k: planes.append((a, k)) or (np.full((1, 6), 5.0), np.zeros((1, 8))))
    # without obstacles: exactly today's calls - the entry is never reached, tau_ext is passed through
    sim = ArmSim(rc)
    sim.send_forces(np.zeros(6))
    assert not seen and not planes and steps[-1]["tau_ext"] is None and sim.link_contact_report() is None
    sim.send_forces(np.zeros(6), tau_ext=np.ones(6))
    assert not seen and np.array_equal(steps[-1]["tau_ext"], np.ones((1, 6)))
    floor = [[0, 0, 1.0, 0.2, 1e4, 50.0, 0.3, 0.01]]
    sim = ArmSim(rc, surfaces=floor)
    sim.send_forces(np.zeros(6))
    assert not seen and len(planes) == 1 and np.array_equal(steps[-1]["tau_ext"], np.full((1, 6), 5.0))
    # with obstacles: the contact first, on the state of the step's start, its torque added to any tau_ext given
    ball = [[0.3, 0.1, 0.4, 0.05, 1e4, 50.0, 0.3]]
    sim = ArmSim(rc, obstacles=ball)
    sim.send_forces(np.zeros(6))
    (a, k), = seen
    assert a[0] == rc.arm_id and a[2].n_obstacles == 1 and tuple(a[2].link_radius)[:6] == (0.04,) * 6
    assert a[5].shape == (1, 1, 7) and np.array_equal(a[3][0], sim.q_init)
    assert np.array_equal(steps[-1]["tau_ext"], np.full((1, 6), 2.0))
    sim.send_forces(np.zeros(6), tau_ext=np.ones(6))
    assert np.array_equal(steps[-1]["tau_ext"], np.full((1, 6), 3.0))
    assert set(sim.link_contact_report()) == {"force", "depth", "n_contacts", "segment", "obstacle", "t"}
    # both: the planes first, then the obstacles, both torques added
    sim = ArmSim(rc, surfaces=floor, obstacles=ball)
    sim.send_forces(np.zeros(6), tau_ext=np.ones(6))
    assert np.array_equal(steps[-1]["tau_ext"], np.full((1, 6), 8.0))
    assert sim.contact_report() is not None and sim.link_contact_report() is not None
    with pytest.raises(ValueError, match="obstacles"):
        ArmSim(rc, obstacles=np.zeros((3, 6))).send_forces(np.zeros(6))


def test_link_contact_fails_loudly_without_gpu_and_runs_with_one():
    from abr_control_amd import AbrkError, device_count
    from abr_control_amd.arms import ArmSim, ur5

    rc = ur5.Config()
    q = np.zeros((2, 6))
    mk = _abi.make_link_contact_params
    if device_count() > 0:
        tau = link_contact.link_contact_step(rc.arm_id, 6, mk(6), q, q, _obstacle(2, 1), None)
        assert tau.shape == (2, 6) and np.isfinite(tau).all()
        sim = ArmSim(rc, obstacles=_obstacle(1, 1)[0])
        sim.send_forces(np.zeros(6))
        assert sim.link_contact_report()["force"].shape == (1, 3)
    else:
        with pytest.raises(AbrkError, match="ENODEV"):
            link_contact.link_contact_step(rc.arm_id, 6, mk(6), q, q, _obstacle(2, 1), None)
        with pytest.raises(AbrkError, match="ENODEV"):
            ArmSim(rc, obstacles=_obstacle(1, 1)[0]).send_forces(np.zeros(6))
