"""C ABI and Python surface of the rigid-body plant (abrk_forward_dynamics_batch, abrk_plant_step_batch, ArmSim): struct
layout, validation before any device use, ENODEV without a device - no GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from abr_control_amd import _abi
from tests.conftest import REPO


def test_plant_params_layout_matches_header(tmp_path):
    src = r'''#include <stdio.h>
#include <stddef.h>
#include "abrk.h"
int main(){printf("%zu %zu %zu %zu\n", sizeof(abrk_plant_params), offsetof(abrk_plant_params, dt),
  offsetof(abrk_plant_params, substeps), offsetof(abrk_plant_params, gravity));return 0;}'''
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-o", exe], input=src.encode(),
                   check=True)
    sizes = [int(v) for v in subprocess.run([exe], capture_output=True, check=True).stdout.split()]
    P = _abi.PlantParams
    assert sizes == [C.sizeof(P), P.dt.offset, P.substeps.offset, P.gravity.offset] == [16, 0, 8, 12]
    p = _abi.make_plant_params(2e-3, substeps=5, gravity=False)
    assert (p.dt, p.substeps, p.gravity) == (2e-3, 5, 0)
    p = _abi.make_plant_params(1e-3)
    assert (p.substeps, p.gravity) == (1, 1)


def test_plant_entry_points_are_exported_and_version_stays():
    from abr_control_amd._lib import lib

    L = lib()
    assert L.abrk_version() == 100
    assert hasattr(L, "abrk_forward_dynamics_batch") and hasattr(L, "abrk_plant_step_batch")


def test_plant_argument_validation_before_device():
    """every rejection of include/abrk.h's plant section, none of which needs a device"""
    from abr_control_amd import AbrkError, engine
    from abr_control_amd._lib import lib

    q = np.zeros((2, 6))
    ok = _abi.make_plant_params(1e-3)
    with pytest.raises(AbrkError, match="ENOARM"):
        engine.forward_dynamics(999, 6, q, q, q)
    with pytest.raises(AbrkError, match="ENOARM"):
        engine.plant_step(999, 6, ok, q.copy(), q.copy(), q)
    for dt in (0.0, -1e-3, np.inf, -np.inf, np.nan):
        with pytest.raises(AbrkError, match="EINVAL"):
            engine.plant_step(0, 6, _abi.make_plant_params(dt), q.copy(), q.copy(), q)
    for sub in (0, -3):
        with pytest.raises(AbrkError, match="EINVAL"):
            engine.plant_step(0, 6, _abi.make_plant_params(1e-3, substeps=sub), q.copy(), q.copy(), q)
    # NULL params, bad dtype code, NULL arrays
    vp = lambda a: C.c_void_p(a.ctypes.data)
    L = lib()
    assert L.abrk_plant_step_batch(0, 0, None, 2, vp(q), vp(q), vp(q), 0, None) == -1
    assert L.abrk_plant_step_batch(0, 7, C.byref(ok), 2, vp(q), vp(q), vp(q), 0, None) == -1
    assert L.abrk_plant_step_batch(0, 0, C.byref(ok), 2, None, vp(q), vp(q), 0, None) == -1
    assert L.abrk_plant_step_batch(0, 0, C.byref(ok), -1, vp(q), vp(q), vp(q), 0, None) == -1
    assert L.abrk_forward_dynamics_batch(0, 0, 2, vp(q), vp(q), vp(q), None, 0, None) == -1
    assert L.abrk_forward_dynamics_batch(0, 7, 2, vp(q), vp(q), vp(q), vp(q), 0, None) == -1
    # wrong shapes / dtypes are caught in Python
    with pytest.raises(ValueError):
        engine.forward_dynamics(0, 6, q, q, np.zeros((2, 5)))
    with pytest.raises(ValueError):
        engine.plant_step(0, 6, ok, q.astype(np.float32), q.copy(), q)  # in/out state of another dtype
    with pytest.raises(TypeError):
        engine.forward_dynamics(0, 6, q, q, q, dtype=np.float16)
    # an empty batch is a no-op even without a device
    e = np.zeros((0, 6))
    assert engine.forward_dynamics(0, 6, e, e, e).shape == (0, 6)
    engine.plant_step(0, 6, ok, e.copy(), e.copy(), e)


def test_plant_fails_loudly_without_gpu():
    from abr_control_amd import AbrkError, device_count, engine
    from abr_control_amd.arms import ArmSim, ur5

    if device_count() > 0:
        pytest.skip("a GPU is present")
    rc = ur5.Config()
    q = np.zeros((2, 6))
    with pytest.raises(AbrkError, match="ENODEV"):
        engine.forward_dynamics(rc.arm_id, 6, q, q, q)
    with pytest.raises(AbrkError, match="ENODEV"):
        engine.plant_step(rc.arm_id, 6, _abi.make_plant_params(1e-3), q.copy(), q.copy(), q)
    with pytest.raises(AbrkError, match="ENODEV"):
        rc.forward_dynamics(np.zeros(6), np.zeros(6), np.zeros(6))
    with pytest.raises(AbrkError, match="ENODEV"):
        ArmSim(rc).send_forces(np.zeros(6))


def test_arm_sim_surface():
    """the reference's ArmSim interface (arms/twojoint/arm_sim.py:20-87) for one state and for B states"""
    from abr_control_amd import arms
    from abr_control_amd.arms import ArmSim, twojoint, ur5

    rc = ur5.Config()
    sim = ArmSim(rc)
    assert (sim.dt, sim.substeps, sim.gravity, sim.t) == (0.001, 1, True, 0.0)
    assert sim.q.shape == (6,) and sim.dq.shape == (6,) and not sim.dq.any()
    assert np.array_equal(sim.q, np.asarray(rc.START_ANGLES, dtype=float))
    for m in ("connect", "disconnect", "reset", "get_feedback", "send_forces"):
        assert callable(getattr(sim, m))
    fb = sim.get_feedback()
    assert set(fb) == {"q", "dq"} and fb["q"] is sim.q and fb["dq"] is sim.dq
    q0 = np.random.RandomState(0).uniform(-1, 1, (5, 6))
    sim = ArmSim(rc, dt=0.002, q_init=q0, substeps=4, gravity=False)
    assert sim.q.shape == (5, 6) and sim.dq.shape == (5, 6) and (sim.substeps, sim.gravity) == (4, False)
    sim.q += 1.0
    sim.dq += 1.0
    sim.connect()
    assert np.array_equal(sim.q, q0) and not sim.dq.any() and sim.q is not sim.q_init
    with pytest.raises(ValueError):
        ArmSim(rc, q_init=np.zeros(5))
    # any BatchedConfig: a user table too
    user = arms.from_table(_abi.load_table("threejoint"), compiled=False)
    assert ArmSim(user, q_init=np.zeros((2, 3))).q.shape == (2, 3)
    # the reference's own two-link closed form keeps its class
    assert twojoint.ArmSim is not ArmSim and "not expected to agree" in twojoint.ArmSim.__doc__
