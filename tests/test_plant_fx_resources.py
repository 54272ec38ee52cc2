"""Register pin of the plant kernel with non-ideal effects (no GPU needed: reads the gfx950 code object the build left in
abr_control_amd/csrc/build/, as tests/test_plant_resources.py does for the plain kernel - skipped where there is no
build).  The UR5 fp64 kernel keeps the plain kernel's register budget: two wavefronts per SIMD (<= 256 registers in all, no AGPRs)
and NO scratch.  It gets there by taking no branch on the effects inside the substep loop and by reading its constants,
its loads and the parked tau where they are consumed (abrk_ctrl.h plant_fx_row; profiles/plant_step.md)."""
import os

import pytest

from tests.test_kernel_resources import BUILD, _table

KERNEL = "plant_fx_kernel<abrk::StaticArm<abrk::Tab_ur5>, double>"
PLAIN = "plant_kernel<abrk::StaticArm<abrk::Tab_ur5>, double>"


@pytest.mark.skipif(not os.path.exists(os.path.join(BUILD, "abrk_arm_ur5.o")), reason="no build in csrc/build")
def test_ur5_plant_fx_kernel_holds_two_waves_per_simd_without_scratch():
    t = _table("abrk_arm_ur5.o")
    assert KERNEL in t, f"{KERNEL} not found in abrk_arm_ur5.o"
    regs, agpr, waves, scratch, lds = t[KERNEL]
    assert scratch == 0 and agpr == 0, t[KERNEL]
    assert regs <= 256 and waves >= 2, t[KERNEL]
    # sin/cos table + wrench slab as the plain kernel (20 KiB), + the parked tau (6 x 64 doubles, 3 KiB) and the
    # constants' table (39 doubles).  NOTE: 23.3 KiB admits six wavefronts per CU of the 160 KiB, not the eight that two
    # waves per SIMD ask for - the registers hold the two-wave budget, the LDS does not (profiles/plant_step.md)
    assert lds <= 24 * 1024, lds
    # the plain kernel beside it is untouched: one symbol, the same budget
    assert PLAIN in t and t[PLAIN][3] == 0 and t[PLAIN][2] >= 2
