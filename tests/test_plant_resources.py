"""Register pin of the plant kernel (no GPU needed: reads the gfx950 code object the build left in
abr_control_amd/csrc/build/, as tests/test_kernel_resources.py reads its kernels - skipped where there is no build).
The plant row is the dynamics pass of the UR5 x,y,z + Coriolis law plus one 6 x 6 solve, so the UR5 fp64 kernel keeps
that law's budget: two wavefronts per SIMD (<= 256 registers in all, no AGPRs) and NO scratch."""
import os

import pytest

from tests.test_kernel_resources import BUILD, _table

KERNEL = "plant_kernel<abrk::StaticArm<abrk::Tab_ur5>, double>"


@pytest.mark.skipif(not os.path.exists(os.path.join(BUILD, "abrk_arm_ur5.o")), reason="no build in csrc/build")
def test_ur5_plant_kernel_holds_two_waves_per_simd_without_scratch():
    t = _table("abrk_arm_ur5.o")
    assert KERNEL in t, f"{KERNEL} not found in abrk_arm_ur5.o"
    regs, agpr, waves, scratch, lds = t[KERNEL]
    assert regs <= 256 and waves >= 2 and scratch == 0 and agpr == 0, t[KERNEL]
    assert lds <= 20 * 1024, lds  # sin/cos table + wrench slab: eight wavefronts per CU fit the 160 KiB
