"""C ABI and Python surface of the plant with non-ideal effects (abrk_forward_dynamics_fx_batch,
abrk_plant_step_fx_batch, _abi.make_plant_effects, ArmSim): struct layout, every rejection of include/abrk.h's effects
section with its message, before any device use - no GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from abr_control_amd import _abi
from tests.conftest import REPO


def test_plant_effects_layout_matches_header(tmp_path):
    fields = ("flags", "damping", "coulomb", "coulomb_vs", "tau_max", "q_min", "q_max", "restitution")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "abrk.h"\nint main(){printf("%zu", '
           'sizeof(abrk_plant_effects));\n'
           + "".join(f'printf(" %zu", offsetof(abrk_plant_effects, {f}));\n' for f in fields)
           + 'printf(" %d %d %d %d\\n", ABRK_FX_SATURATION, ABRK_FX_VISCOUS, ABRK_FX_COULOMB, ABRK_FX_LIMITS);'
             'return 0;}')
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-o", exe], input=src.encode(),
                   check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, check=True).stdout.split()]
    P = _abi.PlantEffects
    assert got[:9] == [C.sizeof(P)] + [getattr(P, f).offset for f in fields]
    assert got[9:] == [_abi.FX_SATURATION, _abi.FX_VISCOUS, _abi.FX_COULOMB, _abi.FX_LIMITS] == [1, 2, 4, 8]


def test_make_plant_effects_broadcasts_and_sets_flags():
    p = _abi.make_plant_effects(6)
    assert p.flags == 0 and p.restitution == 0.0 and not any(p.damping) and not any(p.tau_max)
    p = _abi.make_plant_effects(6, damping=0.5)
    assert p.flags == _abi.FX_VISCOUS and list(p.damping) == [0.5] * 6 + [0.0]
    p = _abi.make_plant_effects(3, coulomb=[0.1, 0.2, 0.3], coulomb_vs=0.01)
    assert p.flags == _abi.FX_COULOMB and list(p.coulomb)[:4] == [0.1, 0.2, 0.3, 0.0] and p.coulomb_vs == 0.01
    p = _abi.make_plant_effects(2, tau_max=12)
    assert p.flags == _abi.FX_SATURATION and list(p.tau_max)[:3] == [12.0, 12.0, 0.0]
    p = _abi.make_plant_effects(6, q_min=-2.0, q_max=np.arange(1, 7), restitution=0.5)
    assert p.flags == _abi.FX_LIMITS and list(p.q_min)[:6] == [-2.0] * 6 and list(p.q_max)[:6] == [1, 2, 3, 4, 5, 6]
    assert p.restitution == 0.5
    p = _abi.make_plant_effects(6, damping=0.5, coulomb=0.3, coulomb_vs=0.01, tau_max=12, q_min=-2, q_max=2)
    assert p.flags == 15
    for bad in (dict(q_min=-2.0), dict(q_max=2.0), dict(coulomb=0.3), dict(damping=[1, 2, 3]),
                dict(tau_max=np.ones((2, 6)))):
        with pytest.raises(ValueError):
            _abi.make_plant_effects(6, **bad)
    with pytest.raises(ValueError):
        _abi.make_plant_effects(8)


def test_plant_fx_entry_points_are_exported_and_version_stays():
    from abr_control_amd._lib import lib

    L = lib()
    assert L.abrk_version() == 100
    assert hasattr(L, "abrk_forward_dynamics_fx_batch") and hasattr(L, "abrk_plant_step_fx_batch")


REJECTED = [
    (dict(damping=-0.1), "damping"),
    (dict(damping=[0.1, 0.1, np.nan, 0.1, 0.1, 0.1]), r"damping\[2\]"),
    (dict(coulomb=-1.0, coulomb_vs=0.01), "coulomb"),
    (dict(coulomb=0.3, coulomb_vs=0.0), "coulomb_vs"),
    (dict(coulomb=0.3, coulomb_vs=-0.01), "coulomb_vs"),
    (dict(coulomb=0.3, coulomb_vs=np.inf), "coulomb_vs"),
    (dict(tau_max=0.0), "tau_max"),
    (dict(tau_max=[12, 12, 12, -1, 12, 12]), r"tau_max\[3\]"),
    (dict(tau_max=np.inf), "tau_max"),
    (dict(q_min=2.0, q_max=2.0), "q_min"),
    (dict(q_min=1.0, q_max=-1.0), "q_min"),
    (dict(q_min=-np.inf, q_max=2.0), "not finite"),
    (dict(q_min=-2.0, q_max=np.nan), "not finite"),
    (dict(q_min=-2.0, q_max=2.0, restitution=1.5), "restitution"),
    (dict(q_min=-2.0, q_max=2.0, restitution=-0.1), "restitution"),
    (dict(restitution=np.nan), "restitution"),
]


@pytest.mark.parametrize("kw,message", REJECTED, ids=[f"{i}-{m[:11]}" for i, (_, m) in enumerate(REJECTED)])
def test_plant_fx_effects_are_validated_before_device(kw, message):
    """every ABRK_EINVAL of the effects struct, through both C entry points, each with its message"""
    from abr_control_amd import AbrkError, engine

    q = np.zeros((2, 6))
    fx = _abi.make_plant_effects(6, **kw)
    with pytest.raises(AbrkError, match="EINVAL") as ei:
        engine.plant_step(0, 6, _abi.make_plant_params(1e-3), q.copy(), q.copy(), q, effects=fx)
    import re

    assert re.search(message, str(ei.value)), str(ei.value)
    with pytest.raises(AbrkError, match=message):
        engine.forward_dynamics(0, 6, q, q, q, effects=fx)


def test_plant_fx_a_non_finite_field_is_refused_with_its_flag_off():
    from abr_control_amd import AbrkError, engine

    q = np.zeros((2, 6))
    fx = _abi.make_plant_effects(6)
    fx.tau_max[1] = np.inf
    with pytest.raises(AbrkError, match="tau_max"):
        engine.forward_dynamics(0, 6, q, q, q, effects=fx)
    fx = _abi.make_plant_effects(6)
    fx.flags = 1 << 7
    with pytest.raises(AbrkError, match="flags"):
        engine.forward_dynamics(0, 6, q, q, q, effects=fx)


def test_plant_fx_argument_validation_before_device():
    from abr_control_amd import AbrkError, engine
    from abr_control_amd._lib import lib

    q = np.zeros((2, 6))
    w = np.zeros((2, 6))
    ok = _abi.make_plant_params(1e-3)
    fx = _abi.make_plant_effects(6, damping=0.5)
    with pytest.raises(AbrkError, match="ENOARM"):
        engine.forward_dynamics(999, 6, q, q, q, effects=fx)
    with pytest.raises(AbrkError, match="ENOARM"):
        engine.plant_step(999, 6, ok, q.copy(), q.copy(), q, wrench=w)
    for dt in (0.0, -1e-3, np.inf, np.nan):
        with pytest.raises(AbrkError, match="EINVAL"):
            engine.plant_step(0, 6, _abi.make_plant_params(dt), q.copy(), q.copy(), q, effects=fx)
    with pytest.raises(AbrkError, match="EINVAL"):
        engine.plant_step(0, 6, _abi.make_plant_params(1e-3, substeps=0), q.copy(), q.copy(), q, tau_ext=q)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    L = lib()
    assert L.abrk_plant_step_fx_batch(0, 0, None, C.byref(fx), 2, vp(q), vp(q), vp(q), None, None, 0, None) == -1
    assert L.abrk_plant_step_fx_batch(0, 7, C.byref(ok), C.byref(fx), 2, vp(q), vp(q), vp(q), None, None, 0, None) == -1
    assert L.abrk_plant_step_fx_batch(0, 0, C.byref(ok), None, 2, None, vp(q), vp(q), None, None, 0, None) == -1
    assert L.abrk_forward_dynamics_fx_batch(0, 0, None, 2, vp(q), vp(q), vp(q), None, None, None, 0, None) == -1
    # shapes are caught in Python
    with pytest.raises(ValueError):
        engine.plant_step(0, 6, ok, q.copy(), q.copy(), q, wrench=np.zeros((2, 5)))
    with pytest.raises(ValueError):
        engine.forward_dynamics(0, 6, q, q, q, tau_ext=np.zeros((3, 6)))
    # an empty batch is a no-op even without a device
    e = np.zeros((0, 6))
    assert engine.forward_dynamics(0, 6, e, e, e, effects=fx, wrench=e).shape == (0, 6)
    engine.plant_step(0, 6, ok, e.copy(), e.copy(), e, effects=fx, tau_ext=e)


def test_plant_fx_fails_loudly_without_gpu():
    from abr_control_amd import AbrkError, device_count, engine
    from abr_control_amd.arms import ArmSim, ur5

    if device_count() > 0:
        pytest.skip("a GPU is present")
    rc = ur5.Config()
    q = np.zeros((2, 6))
    fx = _abi.make_plant_effects(6, damping=0.5)
    with pytest.raises(AbrkError, match="ENODEV"):
        engine.forward_dynamics(rc.arm_id, 6, q, q, q, effects=fx)
    with pytest.raises(AbrkError, match="ENODEV"):
        engine.plant_step(rc.arm_id, 6, _abi.make_plant_params(1e-3), q.copy(), q.copy(), q, wrench=q)
    with pytest.raises(AbrkError, match="ENODEV"):
        ArmSim(rc, effects=fx).send_forces(np.zeros(6), tau_ext=np.zeros(6))


def test_arm_sim_takes_effects():
    from abr_control_amd.arms import ArmSim, ur5

    fx = _abi.make_plant_effects(6, damping=0.5)
    sim = ArmSim(ur5.Config(), effects=fx)
    assert sim.effects is fx and ArmSim(ur5.Config()).effects is None
    import inspect

    assert list(inspect.signature(sim.send_forces).parameters) == ["u", "dt", "tau_ext", "wrench"]
