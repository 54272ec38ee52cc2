"""Resource pin of the whole-arm contact kernel (no GPU needed: reads the gfx950 code objects the build left in
abr_control_amd/csrc/build/, as tests/test_contact_resources.py does - skipped where there is no build).  The row is the
forward kinematics, then per (obstacle, segment) pair a closest point and, behind a branch, the Jacobian columns of that
point: on UR5 and Jaco2 it holds two wavefronts per SIMD without scratch, accumulator registers or LDS in both dtypes;
the fp64 row of a runtime table takes the registers it needs at one wavefront per SIMD, without scratch either
(profiles/link_contact.md has the table).  The kernels beside it keep the budgets their own tests pin."""
import os

import pytest

from tests.test_kernel_resources import BUILD, _table

UR5 = "abrk::StaticArm<abrk::Tab_ur5>"
JACO2 = "abrk::StaticArm<abrk::Tab_jaco2>"


def _need(obj):
    if not os.path.exists(os.path.join(BUILD, obj)):
        pytest.skip("no build in csrc/build")
    return _table(obj)


@pytest.mark.parametrize("obj,arm", (("abrk_arm_ur5.o", UR5), ("abrk_arm_jaco2.o", JACO2)))
def test_ur5_and_jaco2_link_contact_kernels_hold_two_waves_without_scratch(obj, arm):
    t = _need(obj)
    for T in ("double", "float"):
        k = f"link_contact_kernel<{arm}, {T}>"
        assert k in t, f"{k} not found in {obj}"
        regs, agpr, waves, scratch, lds = t[k]
        assert scratch == 0 and agpr == 0 and lds == 0 and waves >= 2 and regs <= 256, (k, t[k])


@pytest.mark.parametrize("obj", ("abrk_arm_rt6.o", "abrk_arm_rt7.o", "abrk_arm_onejoint.o"))
def test_the_link_contact_kernel_is_instantiated_for_every_arm_without_scratch(obj):
    t = _need(obj)
    ks = sorted(k for k in t if k.startswith("link_contact_kernel<"))
    assert len(ks) == 2 and any(k.endswith("double>") for k in ks) and any(k.endswith("float>") for k in ks), (obj, ks)
    for k in ks:
        assert t[k][3] == 0 and t[k][4] == 0, (k, t[k])  # no scratch, no LDS
        if k.endswith("float>"):
            assert t[k][1] == 0 and t[k][2] >= 2, (k, t[k])


def test_the_kernels_beside_it_keep_their_budgets():
    """what tests/test_contact_resources.py, test_force_resources.py and test_plant_payload_resources.py pin, on the
    same objects"""
    t = _need("abrk_arm_ur5.o")
    regs, agpr, waves, scratch, lds = t[f"contact_kernel<{UR5}, double>"]
    assert scratch == 0 and agpr == 0 and waves >= 2 and regs <= 256 and lds == 0
    for T in ("double", "float"):
        regs, agpr, waves, scratch, lds = t[f"force_kernel<{UR5}, {T}>"]
        assert scratch == 0 and agpr == 0 and regs <= 256 and lds == 0
    regs, agpr, waves, scratch, lds = t[f"plant_fx_kernel<{UR5}, double>"]
    assert scratch == 0 and agpr == 0 and regs <= 256 and waves >= 2 and lds <= 24 * 1024
    regs, agpr, waves, scratch, lds = t[f"plant_kernel<{UR5}, double>"]
    assert scratch == 0 and agpr == 0 and regs <= 256 and waves >= 2 and lds <= 20 * 1024
    regs, agpr, waves, scratch, lds = t[f"plant_load_kernel<{UR5}, double>"]
    assert scratch == 0 and waves >= 1 and regs <= 272 and agpr <= 16 and lds <= 33 * 1024 + 512
