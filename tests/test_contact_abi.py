"""C ABI and Python surface of the end-effector contact (abrk_contact_step_batch, contact.contact_step,
ContactSurfaces' plane check, ArmSim(surfaces=...)): the struct's layout, what bad params and a bad host surface array are
refused with - before any device use, naming row and surface - and what the Python layer passes on.  No GPU needed."""
import ctypes as C
import re

import numpy as np
import pytest

from abr_control_amd import _abi, contact


def _surface(B=5, S=2):
    s = np.zeros((B, S, 8))
    s[:, :, 2] = 1.0
    s[:, :, 3:] = [0.1, 1e4, 100.0, 0.5, 0.01]
    return s


def test_contact_struct_layout_and_export():
    from abr_control_amd._lib import lib

    P = _abi.ContactParams
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("frame", 0), ("off", 8), ("n_surfaces", 32),
                                                                   ("vs", 40), ("accumulate", 48)]
    assert C.sizeof(P) == 56
    L = lib()
    assert L.abrk_version() == 100
    assert hasattr(L, "abrk_contact_step_batch") and len(L.abrk_contact_step_batch.argtypes) == 11
    p = _abi.make_contact_params(6)
    assert (p.frame, tuple(p.off), p.n_surfaces, p.vs, p.accumulate) == (13, (0.0, 0.0, 0.0), 1, 1e-3, 0)
    p = _abi.make_contact_params(6, "link2", (0.1, 0.2, 0.3), 4, 0.01, True)
    assert (p.frame, tuple(p.off), p.n_surfaces, p.vs, p.accumulate) == (4, (0.1, 0.2, 0.3), 4, 0.01, 1)
    assert _abi.make_contact_params(6, "joint1").frame == 3
    with pytest.raises(Exception, match="Invalid transformation name"):
        _abi.make_contact_params(6, "joint6")
    with pytest.raises(ValueError, match="offset"):
        _abi.make_contact_params(6, offset=(0, 0))


def test_the_header_no_longer_says_no_contacts():
    import os

    h = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "abrk.h")).read()
    assert "No contacts" not in h and "abrk_contact_step_batch" in h and "ABRK_CONTACT_MAX_SURFACES 4" in h


# (column, value, what the message names)
BAD = [
    (0, 0.5, r"\|n\|"),          # n = (0.5, 0, 1): |n| = 1.118
    (2, 1.0 + 1e-5, r"\|n\|"),   # |n| - 1 = 1e-5 > 1e-6
    (2, 0.0, r"\|n\|"),          # n = 0
    (4, -1.0, r"k=-1"),
    (5, -0.5, r"c=-0\.5"),
    (6, -0.1, r"mu=-0\.1"),
    (7, -1e-3, r"rho=-0\.001"),
    (1, np.nan, r"ny is not finite"),
    (3, np.inf, r"d is not finite"),
    (4, np.inf, r"k is not finite"),
    (7, -np.inf, r"rho is not finite"),
]


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("col,value,message", BAD, ids=[f"{i}" for i in range(len(BAD))])
def test_a_bad_host_surface_is_refused_before_the_device_naming_row_and_surface(col, value, message, dtype):
    from abr_control_amd import AbrkError

    q = np.zeros((5, 6), dtype)
    s = _surface().astype(dtype)
    s[3, 1, col] = value
    with pytest.raises(AbrkError, match="EINVAL") as ei:
        contact.contact_step(0, 6, _abi.make_contact_params(6, n_surfaces=2), q, q, s, None, dtype=dtype)
    msg = str(ei.value)
    assert re.search(message, msg) and "row 3, surface 1" in msg and "surface:" in msg, msg
    # the Python-side check of ContactSurfaces / ArmSim says the same, before it copies anything
    with pytest.raises(ValueError, match="row 3, surface 1"):
        contact.planes_rows(s, 5)


def test_a_normal_within_1e_6_of_unit_length_passes_the_validation():
    """|n| = 1 + 5e-7, zeros of either sign in k, c, mu, rho: what refuses the call afterwards is the missing device"""
    from abr_control_amd import AbrkError, device_count

    q = np.zeros((2, 6))
    s = _surface(2, 1)
    s[0, 0, 2] = 1.0 + 5e-7
    s[1, 0, 4:] = [-0.0, 0.0, -0.0, 0.0]
    contact.planes_rows(s, 2)
    p = _abi.make_contact_params(6)
    if device_count() > 0:
        tau, rep = contact.contact_step(0, 6, p, q, q, s, None, report=True)
        assert tau.shape == (2, 6) and rep.shape == (2, 8)
    else:
        with pytest.raises(AbrkError, match="ENODEV"):
            contact.contact_step(0, 6, p, q, q, s, None)


def test_bad_params_are_einval_before_the_device():
    from abr_control_amd import AbrkError
    from abr_control_amd._lib import lib

    q, s = np.zeros((2, 6)), _surface(2, 1)
    mk = _abi.make_contact_params
    with pytest.raises(AbrkError, match="ENOARM"):
        contact.contact_step(999, 6, mk(6), q, q, s, None)
    for frame in (-1, 14, 99):  # UR5: 0..13
        with pytest.raises(AbrkError, match="EINVAL.*frame"):
            contact.contact_step(0, 6, mk(6, frame), q, q, s, None)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    L, tau = lib(), np.zeros((2, 6))
    for S in (0, 5, -1):
        p = mk(6)
        p.n_surfaces = S
        assert L.abrk_contact_step_batch(0, 0, C.byref(p), 2, vp(q), vp(q), vp(s), vp(tau), None, 0, None) == -1
        assert b"n_surfaces" in L.abrk_last_error()
    for vs in (0.0, -1e-3, np.inf, np.nan):
        with pytest.raises(AbrkError, match="EINVAL.*vs"):
            contact.contact_step(0, 6, mk(6, vs=vs), q, q, s, None)
    with pytest.raises(AbrkError, match="EINVAL.*off"):
        contact.contact_step(0, 6, mk(6, offset=(0, np.nan, 0)), q, q, s, None)
    ok = mk(6)
    assert L.abrk_contact_step_batch(0, 0, None, 2, vp(q), vp(q), vp(s), vp(tau), None, 0, None) == -1
    assert L.abrk_contact_step_batch(0, 7, C.byref(ok), 2, vp(q), vp(q), vp(s), vp(tau), None, 0, None) == -1
    for hole in range(4):  # q, dq, surface and tau are required ...
        args = [vp(q), vp(q), vp(s), vp(tau)]
        args[hole] = None
        assert L.abrk_contact_step_batch(0, 0, C.byref(ok), 2, *args, None, 0, None) == -1
        assert b"required" in L.abrk_last_error()
    # ... a NULL report is accepted: with everything else in order the call goes on to the device (or its absence)
    rc = L.abrk_contact_step_batch(0, 0, C.byref(ok), 2, vp(q), vp(q), vp(s), vp(tau), None, 0, None)
    from abr_control_amd import device_count

    assert rc == (0 if device_count() > 0 else -2)  # ABRK_ENODEV, (rc, L.abrk_last_error())
    # an empty batch is a no-op even without a device, with or without a report
    e = np.zeros((0, 6))
    assert contact.contact_step(0, 6, ok, e, e, np.zeros((0, 1, 8)), None).shape == (0, 6)
    # shape and dtype are caught in Python
    with pytest.raises(ValueError, match="surface"):
        contact.contact_step(0, 6, ok, q, q, np.zeros((2, 2, 8)), None)
    with pytest.raises(ValueError, match="accumulate"):
        contact.contact_step(0, 6, mk(6, accumulate=True), q, q, s, None)


class _Recorder:
    """stands in for the loaded library: records the entry point called and its arguments, returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0

        return call


def test_contact_step_passes_its_arrays_on(monkeypatch):
    fake = _Recorder()
    monkeypatch.setattr(contact, "lib", lambda: fake)
    q, s = np.zeros((3, 6)), _surface(3, 2)
    tau = np.ones((3, 6))
    out = contact.contact_step(0, 6, _abi.make_contact_params(6, n_surfaces=2, accumulate=True), q, q, s, tau)
    name, a = fake.calls[-1]
    assert out is tau and name == "abrk_contact_step_batch" and len(a) == 11
    assert a[3] == 3 and a[6] == s.ctypes.data and a[7] == tau.ctypes.data and a[8] is None
    out, rep = contact.contact_step(0, 6, _abi.make_contact_params(6, n_surfaces=2), q, q, s, None, report=True)
    assert out.shape == (3, 6) and rep.shape == (3, 8) and fake.calls[-1][1][8] == rep.ctypes.data


def test_planes_rows_broadcasts_and_checks_shapes():
    one = _surface(1, 2)[0]
    p = contact.planes_rows(one, 4)
    assert p.shape == (4, 2, 8) and p.flags.c_contiguous and np.array_equal(p[3], one)
    assert contact.planes_rows(_surface(4, 3), 4).shape == (4, 3, 8)
    for bad in (np.zeros(8), np.zeros((2, 7)), _surface(3, 2), np.zeros((4, 5, 8)), np.zeros((0, 8))):
        with pytest.raises(ValueError, match="planes"):
            contact.planes_rows(bad, 4)
    d = contact.report_dict(np.arange(16.0).reshape(2, 8))
    assert np.array_equal(d["force"], [[0, 1, 2], [8, 9, 10]]) and np.array_equal(d["force_local"][0], [3, 4, 5])
    assert np.array_equal(d["depth"], [6, 14]) and d["n_contacts"].tolist() == [7, 15]


def test_arm_sim_takes_surfaces(monkeypatch):
    from abr_control_amd import plant_payload
    from abr_control_amd.arms import ArmSim, ur5

    rc = ur5.Config()
    seen, steps = [], []
    monkeypatch.setattr(plant_payload, "plant_step", lambda *a, **k: steps.append(k))
    # without surfaces: exactly today's calls - the contact entry is never reached, tau_ext is passed through
    monkeypatch.setattr(contact, "contact_step", lambda *a, **k: seen.append((a, k)) or (np.full((1, 6), 2.0), np.zeros((1, 8))))
    sim = ArmSim(rc)
    sim.send_forces(np.zeros(6))
    assert not seen and steps[-1]["tau_ext"] is None and sim.contact_report() is None
    sim.send_forces(np.zeros(6), tau_ext=np.ones(6))
    assert not seen and np.array_equal(steps[-1]["tau_ext"], np.ones((1, 6)))
    # with surfaces: the contact first, on the state of the step's start, its torque added to any tau_ext given
    floor = [[0, 0, 1.0, 0.2, 1e4, 50.0, 0.3, 0.01]]
    sim = ArmSim(rc, surfaces=floor)
    sim.send_forces(np.zeros(6))
    (a, k), = seen
    assert a[0] == rc.arm_id and a[2].n_surfaces == 1 and a[2].frame == 13 and a[5].shape == (1, 1, 8)
    assert np.array_equal(a[3][0], sim.q_init) and np.array_equal(steps[-1]["tau_ext"], np.full((1, 6), 2.0))
    sim.send_forces(np.zeros(6), tau_ext=np.ones(6))
    assert np.array_equal(steps[-1]["tau_ext"], np.full((1, 6), 3.0))
    assert set(sim.contact_report()) == {"force", "force_local", "depth", "n_contacts"}
    with pytest.raises(ValueError, match="planes"):
        ArmSim(rc, surfaces=np.zeros((3, 7))).send_forces(np.zeros(6))


def test_contact_fails_loudly_without_gpu_and_runs_with_one():
    from abr_control_amd import AbrkError, device_count
    from abr_control_amd.arms import ArmSim, ur5

    rc = ur5.Config()
    q = np.zeros((2, 6))
    if device_count() > 0:
        tau = contact.contact_step(rc.arm_id, 6, _abi.make_contact_params(6), q, q, _surface(2, 1), None)
        assert tau.shape == (2, 6) and np.isfinite(tau).all()
        sim = ArmSim(rc, surfaces=_surface(1, 1)[0])
        sim.send_forces(np.zeros(6))
        assert sim.contact_report()["force"].shape == (1, 3)
    else:
        with pytest.raises(AbrkError, match="ENODEV"):
            contact.contact_step(rc.arm_id, 6, _abi.make_contact_params(6), q, q, _surface(2, 1), None)
        with pytest.raises(AbrkError, match="ENODEV"):
            ArmSim(rc, surfaces=_surface(1, 1)[0]).send_forces(np.zeros(6))
