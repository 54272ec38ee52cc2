"""Resource pin of the end-effector contact kernel (no GPU needed: reads the gfx950 code objects the build left in
abr_control_amd/csrc/build/, as tests/test_loop_trace_resources.py does - skipped where there is no build).  The row is
the forward kinematics, the point Jacobian and a few dozen operations per surface: two wavefronts per SIMD without
scratch, accumulator registers or LDS (profiles/contact_step.md has the table).  The kernels beside it - the three plant
kernels and the recorder's - keep the budgets their own tests pin."""
import os

import pytest

from tests.test_kernel_resources import BUILD, _table

UR5 = "abrk::StaticArm<abrk::Tab_ur5>"


def _need(obj):
    if not os.path.exists(os.path.join(BUILD, obj)):
        pytest.skip("no build in csrc/build")
    return _table(obj)


def test_ur5_contact_kernels_hold_two_waves_without_scratch():
    t = _need("abrk_arm_ur5.o")
    for T in ("double", "float"):
        k = f"contact_kernel<{UR5}, {T}>"
        assert k in t, f"{k} not found in abrk_arm_ur5.o"
        regs, agpr, waves, scratch, lds = t[k]
        assert scratch == 0 and agpr == 0 and waves >= 2 and regs <= 256, (k, t[k])
        assert lds == 0, (k, lds)


@pytest.mark.parametrize("obj", ("abrk_arm_jaco2.o", "abrk_arm_rt6.o"))
def test_the_contact_kernel_is_instantiated_for_general_chains_and_runtime_tables(obj):
    t = _need(obj)
    ks = sorted(k for k in t if k.startswith("contact_kernel<"))
    assert len(ks) == 2 and any(k.endswith("double>") for k in ks) and any(k.endswith("float>") for k in ks), (obj, ks)
    for k in ks:
        assert t[k][3] == 0, (k, t[k])  # no scratch


def test_the_kernels_beside_it_keep_their_budgets():
    """what tests/test_plant_payload_resources.py and tests/test_loop_trace_resources.py pin, on the same objects"""
    t = _need("abrk_arm_ur5.o")
    regs, agpr, waves, scratch, lds = t[f"plant_load_kernel<{UR5}, double>"]
    assert scratch == 0 and waves >= 1 and regs <= 272 and agpr <= 16 and lds <= 33 * 1024 + 512
    regs, agpr, waves, scratch, lds = t[f"plant_load_kernel<{UR5}, float>"]
    assert scratch == 0 and agpr == 0 and regs <= 256 and waves >= 2 and lds <= 17 * 1024
    regs, agpr, waves, scratch, lds = t[f"plant_fx_kernel<{UR5}, double>"]
    assert scratch == 0 and agpr == 0 and regs <= 256 and waves >= 2 and lds <= 24 * 1024
    regs, agpr, waves, scratch, lds = t[f"plant_kernel<{UR5}, double>"]
    assert scratch == 0 and agpr == 0 and regs <= 256 and waves >= 2 and lds <= 20 * 1024
    for obj, arm in (("abrk_arm_ur5.o", "ur5"), ("abrk_arm_jaco2.o", "jaco2")):
        regs, agpr, waves, scratch, lds = _need(obj)[f"trace_kernel<abrk::StaticArm<abrk::Tab_{arm}>, double>"]
        assert waves >= 2 and scratch == 0 and agpr == 0 and lds <= 16 * 1024
