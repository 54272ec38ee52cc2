"""C ABI and Python surface of the plant with a payload at the end effector (abrk_forward_dynamics_payload_batch,
abrk_plant_step_payload_batch, plant_payload.forward_dynamics / plant_step, ArmSim(payload=...)): what is exported,
what a bad host payload array is refused with - before any device use - and what the Python layer passes on.  No GPU
needed."""
import ctypes as C

import numpy as np
import pytest

from abr_control_amd import _abi, plant_payload


def test_plant_payload_entry_points_are_exported_and_version_stays():
    from abr_control_amd._lib import lib

    L = lib()
    assert L.abrk_version() == 100
    assert hasattr(L, "abrk_forward_dynamics_payload_batch") and hasattr(L, "abrk_plant_step_payload_batch")
    assert len(L.abrk_forward_dynamics_payload_batch.argtypes) == len(L.abrk_forward_dynamics_fx_batch.argtypes) + 1
    assert len(L.abrk_plant_step_payload_batch.argtypes) == len(L.abrk_plant_step_fx_batch.argtypes) + 1


def _payload(B=5):
    p = np.zeros((B, 4))
    p[:, 0] = 1.0
    p[:, 1:] = 0.05
    return p


BAD = [
    (0, -0.5, r"row 3.*m=-0\.5"),
    (0, np.nan, r"row 3.*m="),
    (0, np.inf, r"row 3.*m="),
    (1, np.nan, r"row 3.*rx="),
    (2, -np.inf, r"row 3.*ry="),
    (3, np.inf, r"row 3.*rz="),
]


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("col,value,message", BAD, ids=[f"{i}" for i in range(len(BAD))])
def test_a_bad_host_payload_is_refused_before_the_device_naming_the_row(col, value, message, dtype):
    import re

    from abr_control_amd import AbrkError, engine

    q = np.zeros((5, 6), dtype)
    p = _payload().astype(dtype)
    p[3, col] = value
    with pytest.raises(AbrkError, match="EINVAL") as ei:
        plant_payload.plant_step(0, 6, _abi.make_plant_params(1e-3), q.copy(), q.copy(), q, dtype=dtype, payload=p)
    assert re.search(message, str(ei.value)) and "payload" in str(ei.value), str(ei.value)
    with pytest.raises(AbrkError, match=message):
        plant_payload.forward_dynamics(0, 6, q, q, q, dtype=dtype, payload=p)


def test_a_zero_mass_of_either_sign_is_accepted_by_the_validation():
    """m = +0 and m = -0 pass the payload check: what refuses the call afterwards is the missing device (or nothing)"""
    from abr_control_amd import AbrkError, device_count, engine

    q = np.zeros((2, 6))
    p = np.array([[0.0, 0, 0, 0], [-0.0, 0.1, 0, 0]])
    if device_count() > 0:
        assert plant_payload.forward_dynamics(0, 6, q, q, q, payload=p).shape == (2, 6)
    else:
        with pytest.raises(AbrkError, match="ENODEV"):
            plant_payload.forward_dynamics(0, 6, q, q, q, payload=p)


def test_plant_payload_argument_validation_before_device():
    from abr_control_amd import AbrkError, engine
    from abr_control_amd._lib import lib

    q = np.zeros((2, 6))
    p = _payload(2)
    ok = _abi.make_plant_params(1e-3)
    with pytest.raises(AbrkError, match="ENOARM"):
        plant_payload.forward_dynamics(999, 6, q, q, q, payload=p)
    with pytest.raises(AbrkError, match="ENOARM"):
        plant_payload.plant_step(999, 6, ok, q.copy(), q.copy(), q, payload=p)
    for dt in (0.0, -1e-3, np.inf, np.nan):
        with pytest.raises(AbrkError, match="EINVAL"):
            plant_payload.plant_step(0, 6, _abi.make_plant_params(dt), q.copy(), q.copy(), q, payload=p)
    with pytest.raises(AbrkError, match="EINVAL"):
        plant_payload.plant_step(0, 6, _abi.make_plant_params(1e-3, substeps=0), q.copy(), q.copy(), q, payload=p)
    # the effects are still checked, ahead of the payload
    with pytest.raises(AbrkError, match="damping"):
        plant_payload.forward_dynamics(0, 6, q, q, q, effects=_abi.make_plant_effects(6, damping=-1.0), payload=p)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    L = lib()
    assert L.abrk_plant_step_payload_batch(0, 0, None, None, 2, vp(q), vp(q), vp(q), None, None, vp(p), 0, None) == -1
    assert L.abrk_plant_step_payload_batch(0, 7, C.byref(ok), None, 2, vp(q), vp(q), vp(q), None, None, vp(p), 0,
                                           None) == -1
    assert L.abrk_plant_step_payload_batch(0, 0, C.byref(ok), None, 2, None, vp(q), vp(q), None, None, vp(p), 0,
                                           None) == -1
    assert L.abrk_forward_dynamics_payload_batch(0, 0, None, 2, vp(q), vp(q), vp(q), None, None, vp(p), None, 0,
                                                 None) == -1
    # shape and dtype are caught in Python
    with pytest.raises(ValueError, match="payload"):
        plant_payload.plant_step(0, 6, ok, q.copy(), q.copy(), q, payload=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="payload"):
        plant_payload.forward_dynamics(0, 6, q, q, q, payload=np.zeros((3, 4)))
    # (a host array of another type is converted like every host input; a DeviceArray must have the call's type)
    from abr_control_amd._lib import DeviceArray

    def fake_device_array(shape, dtype):
        d = DeviceArray.__new__(DeviceArray)
        d.shape, d.dtype, d.device, d.nbytes, d.ptr, d._base = shape, np.dtype(dtype), 0, 0, 0x1000, d
        return d

    qd = fake_device_array((2, 6), np.float64)
    with pytest.raises(ValueError, match="payload"):
        plant_payload.forward_dynamics(0, 6, qd, qd, qd, payload=fake_device_array((2, 4), np.float32))
    with pytest.raises(ValueError, match="payload"):
        plant_payload.plant_step(0, 6, ok, qd, qd, qd, payload=fake_device_array((3, 4), np.float64))
    with pytest.raises(TypeError, match="mixing"):
        plant_payload.plant_step(0, 6, ok, qd, qd, qd, payload=p)
    # an empty batch is a no-op even without a device
    e = np.zeros((0, 6))
    assert plant_payload.forward_dynamics(0, 6, e, e, e, payload=np.zeros((0, 4))).shape == (0, 6)
    plant_payload.plant_step(0, 6, ok, e.copy(), e.copy(), e, payload=np.zeros((0, 4)))


class _Recorder:
    """stands in for the loaded library: records the entry point called and its arguments, returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0

        return call


def test_payload_none_makes_the_calls_made_today(monkeypatch):
    from abr_control_amd import engine

    fake = _Recorder()
    monkeypatch.setattr(engine, "lib", lambda: fake)
    q, w, p = np.zeros((3, 6)), np.zeros((3, 6)), _payload(3)
    ok = _abi.make_plant_params(1e-3)
    fx = _abi.make_plant_effects(6, damping=0.5)
    engine.forward_dynamics(0, 6, q, q, q)
    plant_payload.forward_dynamics(0, 6, q, q, q, payload=None)
    plant_payload.plant_step(0, 6, ok, q.copy(), q.copy(), q, payload=None)
    plant_payload.plant_step(0, 6, ok, q.copy(), q.copy(), q, effects=fx, wrench=w, payload=None)
    plant_payload.forward_dynamics(0, 6, q, q, q, tau_ext=q, payload=None)
    assert [c[0] for c in fake.calls] == ["abrk_forward_dynamics_batch", "abrk_forward_dynamics_batch",
                                          "abrk_plant_step_batch", "abrk_plant_step_fx_batch",
                                          "abrk_forward_dynamics_fx_batch"]
    assert [len(c[1]) for c in fake.calls] == [9, 9, 9, 12, 12]
    fake.calls.clear()
    # with a payload: the payload entries, the array last among the inputs; effects, tau_ext and wrench stay optional
    plant_payload.plant_step(0, 6, ok, q.copy(), q.copy(), q, payload=p)
    name, a = fake.calls[-1]
    assert name == "abrk_plant_step_payload_batch" and len(a) == 13
    assert a[3] is None and a[8] is None and a[9] is None and a[10] == p.ctypes.data
    ddq = plant_payload.forward_dynamics(0, 6, q, q, q, effects=fx, wrench=w, payload=p)
    name, a = fake.calls[-1]
    assert name == "abrk_forward_dynamics_payload_batch" and len(a) == 13
    assert a[7] is None and a[8] == w.ctypes.data and a[9] == p.ctypes.data and a[10] == ddq.ctypes.data


def test_arm_sim_takes_a_payload(monkeypatch):
    from abr_control_amd import engine
    from abr_control_amd.arms import ArmSim, ur5

    rc = ur5.Config()
    assert ArmSim(rc).payload is None
    sim = ArmSim(rc, payload=(1.5, [0.0, 0.02, 0.1]))
    assert np.array_equal(sim.payload, [1.5, 0.0, 0.02, 0.1])
    rows = np.array([[1.0, 0, 0, 0.1], [2.0, 0, 0, 0.1], [0.0, 0, 0, 0]])
    many = ArmSim(rc, q_init=np.zeros((3, 6)), payload=rows)
    assert np.array_equal(many.payload, rows)
    for bad in ((1.0, [0.0, 0.1]), np.zeros(3), np.zeros((3, 5))):
        with pytest.raises(ValueError, match="payload"):
            ArmSim(rc, payload=bad)
    seen = []
    monkeypatch.setattr(plant_payload, "plant_step", lambda *a, **k: seen.append(k))
    sim.send_forces(np.zeros(6))
    assert seen[-1]["payload"].shape == (1, 4) and np.array_equal(seen[-1]["payload"][0], [1.5, 0.0, 0.02, 0.1])
    many.send_forces(np.zeros((3, 6)))
    assert np.array_equal(seen[-1]["payload"], rows)
    many.set_payload((0.5, [0, 0, 0]))  # from here on, one payload for every arm
    many.send_forces(np.zeros((3, 6)))
    assert np.array_equal(seen[-1]["payload"], np.tile([0.5, 0, 0, 0], (3, 1)))
    many.set_payload(None)
    many.send_forces(np.zeros((3, 6)))
    assert seen[-1]["payload"] is None


def test_plant_payload_fails_loudly_without_gpu():
    from abr_control_amd import AbrkError, device_count, engine
    from abr_control_amd.arms import ArmSim, ur5

    if device_count() > 0:
        pytest.skip("a GPU is present")
    rc = ur5.Config()
    q = np.zeros((2, 6))
    p = _payload(2)
    with pytest.raises(AbrkError, match="ENODEV"):
        plant_payload.forward_dynamics(rc.arm_id, 6, q, q, q, payload=p)
    with pytest.raises(AbrkError, match="ENODEV"):
        plant_payload.plant_step(rc.arm_id, 6, _abi.make_plant_params(1e-3), q.copy(), q.copy(), q, payload=p)
    with pytest.raises(AbrkError, match="ENODEV"):
        ArmSim(rc, payload=(1.0, [0, 0, 0.1])).send_forces(np.zeros(6))
