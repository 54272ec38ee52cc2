"""C ABI and Python surface of the force-control law (abrk_force_control_batch, force_control.force_control_step,
ForceController's command check): the struct's layout, what bad params and a bad host cmd array are refused with - before
any device use, naming the row - and what the Python layer passes on.  No GPU needed.  (The layout is also exercised end
to end by tests/test_force_hostsim.py, whose host build reads the ctypes struct as include/abrk.h declares it.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from abr_control_amd import _abi, force_control

GAINS = ("kp", "kv", "kf", "ki", "i_max", "kvf", "f_touch", "v_app", "kv_null")


def _inputs(B=5, n=6, dtype=np.float64):
    q = np.zeros((B, n), dtype)
    cmd = np.zeros((B, 4), dtype)
    cmd[:, 2], cmd[:, 3] = 1.0, 10.0
    return dict(q=q, dq=q, target=np.zeros((B, 6), dtype), cmd=cmd, force=np.zeros((B, 3), dtype),
                integ=np.zeros(B, dtype))


def _step(params, dtype=np.float64, arm=0, n=6, B=5, **over):
    a = dict(_inputs(B, n, dtype), **over)
    return force_control.force_control_step(arm, n, params, a["q"], a["dq"], a["target"], a["cmd"], a["force"],
                                            a["integ"], u=a.get("u"), target_velocity=a.get("tv"), dtype=dtype)


def test_force_struct_layout_and_export():
    from abr_control_amd._lib import lib

    P = _abi.ForceParams
    want = [("frame", 0), ("off", 8)] + [(k, 32 + 8 * i) for i, k in enumerate(GAINS)] + [
        ("dt", 104), ("use_g", 112), ("accumulate", 116), ("force_ld", 120)]
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == want
    assert C.sizeof(P) == 128
    L = lib()
    assert hasattr(L, "abrk_force_control_batch") and len(L.abrk_force_control_batch.argtypes) == 14
    p = _abi.make_force_params(6)
    assert (p.frame, tuple(p.off), p.dt, p.use_g, p.accumulate, p.force_ld) == (13, (0.0, 0.0, 0.0), 1e-3, 1, 0, 3)
    assert [getattr(p, k) for k in GAINS] == [100.0, 20.0, 0.5, 20.0, 50.0, 20.0, 0.5, 0.05, 10.0]
    p = _abi.make_force_params(6, "link2", (0.1, 0.2, 0.3), kp=1, kv=2, kf=3, ki=4, i_max=5, kvf=6, f_touch=7, v_app=8,
                               kv_null=9, dt=0.01, use_g=False, accumulate=True, force_ld=8)
    assert (p.frame, tuple(p.off), p.dt, p.use_g, p.accumulate, p.force_ld) == (4, (0.1, 0.2, 0.3), 0.01, 0, 1, 8)
    assert [getattr(p, k) for k in GAINS] == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    with pytest.raises(Exception, match="Invalid transformation name"):
        _abi.make_force_params(6, "joint6")
    with pytest.raises(ValueError, match="offset"):
        _abi.make_force_params(6, offset=(0, 0))


def test_the_header_and_the_design_state_the_law():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    h = open(os.path.join(root, "include", "abrk.h")).read()
    assert "abrk_force_control_batch" in h and "typedef struct abrk_force_params" in h
    for word in ("INTO FREE SPACE", "NOT MODELLED", "orientation", "Coriolis", "a moment about the point",
                 "more than one\n * constrained direction", "A DEVICE array is NOT validated"):
        assert word in h, word
    d = open(os.path.join(root, "DESIGN.md")).read()
    assert "any force-control law" not in d and "abrk_force_control_batch" in d


# (column, value, what the message names)
BAD = [
    (0, 0.5, r"\|n\|"),          # n = (0.5, 0, 1)
    (2, 1.0 + 1e-5, r"\|n\|"),   # |n| - 1 = 1e-5 > 1e-6
    (2, 0.0, r"\|n\|"),          # n = 0
    (3, -1.0, r"f_des=-1"),
    (1, np.nan, r"ny is not finite"),
    (2, np.inf, r"nz is not finite"),
    (3, np.inf, r"f_des is not finite"),
    (3, np.nan, r"f_des is not finite"),
]


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("col,value,message", BAD, ids=[f"{i}" for i in range(len(BAD))])
def test_a_bad_host_cmd_is_refused_before_the_device_naming_the_row(col, value, message, dtype):
    from abr_control_amd import AbrkError

    cmd = _inputs(dtype=dtype)["cmd"].copy()
    cmd[3, col] = value
    with pytest.raises(AbrkError, match="EINVAL") as ei:
        _step(_abi.make_force_params(6), dtype, cmd=cmd)
    msg = str(ei.value)
    assert re.search(message, msg) and "row 3" in msg and "cmd:" in msg, msg
    # the Python-side check of ForceController says the same, before it copies anything
    with pytest.raises(ValueError, match="row 3"):
        force_control.command_rows(cmd[:, :3], cmd[:, 3], 5)


def _goes_on_to_the_device(call):
    """with everything in order the call reaches the device, or its absence"""
    from abr_control_amd import AbrkError, device_count

    if device_count() > 0:
        return call()
    with pytest.raises(AbrkError, match="ENODEV"):
        call()


def test_a_normal_within_1e_6_of_unit_length_and_a_zero_force_pass_the_validation():
    cmd = _inputs(2)["cmd"].copy()
    cmd[0, 2] = 1.0 + 5e-7
    cmd[1, 3] = -0.0
    force_control.command_rows(cmd[:, :3], cmd[:, 3], 2)
    _goes_on_to_the_device(lambda: _step(_abi.make_force_params(6), B=2, cmd=cmd))


def test_bad_params_are_einval_before_the_device():
    from abr_control_amd import AbrkError
    from abr_control_amd._lib import lib

    mk = _abi.make_force_params
    with pytest.raises(AbrkError, match="ENOARM"):
        _step(mk(6), arm=999)
    for frame in (-1, 14, 99):  # UR5: 0..13
        with pytest.raises(AbrkError, match="EINVAL.*frame"):
            _step(mk(6, frame))
    for k in GAINS:
        for bad in (-1e-3, np.inf, np.nan):
            with pytest.raises(AbrkError, match=f"EINVAL.*{k}=") as ei:
                _step(mk(6, **{k: bad}))
            assert "is not a finite value >= 0" in str(ei.value)
    for dt in (0.0, -1e-3, np.inf, np.nan):
        with pytest.raises(AbrkError, match="EINVAL.*dt="):
            _step(mk(6, dt=dt))
    for ld in (2, 1, 0):
        with pytest.raises(AbrkError, match="EINVAL.*force_ld"):
            _step(mk(6, force_ld=ld), force=np.zeros((5, ld)))
    with pytest.raises(AbrkError, match="EINVAL.*off"):
        _step(mk(6, offset=(0, np.nan, 0)))
    # zeros of either sign are gains like any other
    zero = mk(6, **{k: -0.0 for k in GAINS})
    _goes_on_to_the_device(lambda: _step(zero))
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    L, a, u = lib(), _inputs(2), np.zeros((2, 6))
    ok = mk(6)
    arrays = [a["q"], a["dq"], a["target"], None, a["cmd"], a["force"], a["integ"], u]
    ptrs = [None if x is None else vp(x) for x in arrays]
    assert L.abrk_force_control_batch(0, 0, None, 2, *ptrs, 0, None) == -1
    assert L.abrk_force_control_batch(0, 7, C.byref(ok), 2, *ptrs, 0, None) == -1
    for hole in (0, 1, 2, 4, 5, 6, 7):  # everything but target_velocity is required ...
        args = list(ptrs)
        args[hole] = None
        assert L.abrk_force_control_batch(0, 0, C.byref(ok), 2, *args, 0, None) == -1
        assert b"required" in L.abrk_last_error()
    # ... a NULL target_velocity is accepted: the call goes on to the device (or its absence)
    from abr_control_amd import device_count

    rc = L.abrk_force_control_batch(0, 0, C.byref(ok), 2, *ptrs, 0, None)
    assert rc == (0 if device_count() > 0 else -2), (rc, L.abrk_last_error())  # ABRK_ENODEV
    # an empty batch is a no-op even without a device
    assert _step(ok, B=0).shape == (0, 6)
    # shape and dtype are caught in Python
    with pytest.raises(ValueError, match="cmd"):
        _step(ok, cmd=np.zeros((5, 3)))
    with pytest.raises(ValueError, match="force"):
        _step(mk(6, force_ld=8))
    with pytest.raises(ValueError, match="integ"):
        _step(ok, integ=np.zeros((5, 1)))
    with pytest.raises(ValueError, match="integ"):
        _step(ok, integ=None)
    with pytest.raises(ValueError, match="accumulate"):
        _step(mk(6, accumulate=True))


class _Recorder:
    """stands in for the loaded library: records the entry point called and its arguments, returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0

        return call


def test_force_control_step_passes_its_arrays_on(monkeypatch):
    fake = _Recorder()
    monkeypatch.setattr(force_control, "lib", lambda: fake)
    a = _inputs(3)
    u, tv = np.ones((3, 6)), np.zeros((3, 6))
    wide = np.zeros((3, 8))
    out = _step(_abi.make_force_params(6, accumulate=True, force_ld=8), B=3, u=u, tv=tv, force=wide, **{
        k: a[k] for k in ("cmd", "integ")})
    name, args = fake.calls[-1]
    assert out is u and name == "abrk_force_control_batch" and len(args) == 14
    assert args[3] == 3 and args[7] == tv.ctypes.data and args[8] == a["cmd"].ctypes.data
    assert args[9] == wide.ctypes.data and args[10] == a["integ"].ctypes.data and args[11] == u.ctypes.data
    out = _step(_abi.make_force_params(6), B=3)
    assert out.shape == (3, 6) and fake.calls[-1][1][7] is None and fake.calls[-1][1][11] == out.ctypes.data


def test_command_rows_broadcasts_and_checks_shapes():
    c = force_control.command_rows((0, 0, 1), 10.0, 4)
    assert c.shape == (4, 4) and c.flags.c_contiguous and np.array_equal(c[3], [0, 0, 1, 10])
    n = np.tile([[1.0, 0, 0]], (4, 1))
    c = force_control.command_rows(n, [1, 2, 3, 4], 4)
    assert np.array_equal(c[:, 0], np.ones(4)) and np.array_equal(c[:, 3], [1, 2, 3, 4])
    for normal, f in (((0, 1), 1.0), (np.zeros((3, 3)), 1.0), ((0, 0, 1), [1, 2])):
        with pytest.raises(ValueError, match="normal has shape"):
            force_control.command_rows(normal, f, 4)


def test_the_package_exports_the_controller_and_it_fails_loudly_without_gpu():
    import abr_control_amd as a
    from abr_control_amd.arms import ur5

    assert a.ForceController is force_control.ForceController
    rc = ur5.Config()
    with pytest.raises(TypeError, match="unknown gain"):
        a.ForceController(rc, 4, (0, 0, 1), 10.0, kq=3)
    with pytest.raises(ValueError, match="row 0"):
        a.ForceController(rc, 4, (0, 0, 2), 10.0)
    with pytest.raises(ValueError, match="f_des=-1"):
        a.ForceController(rc, 4, (0, 0, 1), -1.0)
    if a.device_count() > 0:
        fc = a.ForceController(rc, 4, (0, 0, 1), 10.0, kp=50.0)
        assert set(fc.device_arrays()) == {"cmd", "integ", "u"} and fc.params(8).force_ld == 8 and fc.params(3).kp == 50
    else:
        with pytest.raises(a.AbrkError):
            a.ForceController(rc, 4, (0, 0, 1), 10.0)
