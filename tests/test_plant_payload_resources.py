"""Resource pin of the plant kernel with a payload at the end effector (no GPU needed: reads the gfx950 code object the
build left in abr_control_amd/csrc/build/, as tests/test_plant_fx_resources.py does - skipped where there is no build).
What the build achieves on the UR5 (profiles/plant_step.md has the table and the forms tried):
  fp64: NO scratch, in the ONE-wave form - 260 registers (4 of them AGPRs) against the 256 of two waves per SIMD, and
        32.3 KiB of LDS (the effects kernel's 23.3 KiB + 9 KiB where sqrt(m) Jp waits for the dynamics pass), which
        admits four wavefronts per CU of the 160 KiB: one per SIMD either way;
  fp32: NO scratch, two waves per SIMD, 16.2 KiB of LDS (nine wavefronts per CU).
The two kernels beside it keep their symbols and budgets."""
import os

import pytest

from tests.test_kernel_resources import BUILD, _table

ARM = "abrk::StaticArm<abrk::Tab_ur5>"
LOAD64, LOAD32 = f"plant_load_kernel<{ARM}, double>", f"plant_load_kernel<{ARM}, float>"
FX64, PLAIN64 = f"plant_fx_kernel<{ARM}, double>", f"plant_kernel<{ARM}, double>"


@pytest.mark.skipif(not os.path.exists(os.path.join(BUILD, "abrk_arm_ur5.o")), reason="no build in csrc/build")
def test_ur5_plant_load_kernels_use_no_scratch():
    t = _table("abrk_arm_ur5.o")
    assert LOAD64 in t and LOAD32 in t, "plant_load_kernel not found in abrk_arm_ur5.o"
    regs, agpr, waves, scratch, lds = t[LOAD64]
    assert scratch == 0, t[LOAD64]
    assert waves >= 1 and regs <= 272 and agpr <= 16, t[LOAD64]  # the one-wave form, within a few registers of two
    assert lds <= 33 * 1024 + 512, lds  # four wavefronts per CU (160 KiB / 32.3 KiB)
    regs, agpr, waves, scratch, lds = t[LOAD32]
    assert scratch == 0 and agpr == 0 and regs <= 256 and waves >= 2, t[LOAD32]
    assert lds <= 17 * 1024, lds
    # the two existing kernels: present, each with its budget
    regs, agpr, waves, scratch, lds = t[FX64]
    assert scratch == 0 and agpr == 0 and regs <= 256 and waves >= 2 and lds <= 24 * 1024, t[FX64]
    regs, agpr, waves, scratch, lds = t[PLAIN64]
    assert scratch == 0 and agpr == 0 and regs <= 256 and waves >= 2 and lds <= 20 * 1024, t[PLAIN64]


@pytest.mark.skipif(not os.path.exists(os.path.join(BUILD, "abrk_arm_jaco2.o")), reason="no build in csrc/build")
def test_the_payload_kernel_is_instantiated_beside_the_effects_kernel():
    """general chains (jaco2) and runtime tables (six joints), both types: where plant_fx_kernel is, plant_load_kernel is"""
    for obj in ("abrk_arm_jaco2.o", "abrk_arm_rt6.o"):
        t = _table(obj)
        fx = sorted(k for k in t if k.startswith("plant_fx_kernel<"))
        load = sorted(k for k in t if k.startswith("plant_load_kernel<"))
        assert len(fx) == 2 and [k.replace("plant_fx_kernel", "plant_load_kernel") for k in fx] == load, (obj, fx, load)
        for k in load:
            assert t[k][3] == 0, (k, t[k])  # no scratch
