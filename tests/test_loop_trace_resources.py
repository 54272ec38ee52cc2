"""Register pin of the loop recorder's kernel (no GPU needed: reads the gfx950 code objects the build left in
abr_control_amd/csrc/build/, as tests/test_plant_resources.py does - skipped where there is no build).  The row is the
forward kinematics, six loads and a handful of stores: nothing in it has a reason to use scratch or accumulator registers,
or to drop below two wavefronts per SIMD."""
import os

import pytest

from tests.test_kernel_resources import BUILD, _table


@pytest.mark.parametrize("arm", ("ur5", "jaco2"))
def test_trace_kernel_holds_two_waves_per_simd_without_scratch(arm):
    obj = f"abrk_arm_{arm}.o"
    if not os.path.exists(os.path.join(BUILD, obj)):
        pytest.skip("no build in csrc/build")
    kernel = f"trace_kernel<abrk::StaticArm<abrk::Tab_{arm}>, double>"
    t = _table(obj)
    assert kernel in t, f"{kernel} not found in {obj}"
    regs, agpr, waves, scratch, lds = t[kernel]
    assert waves >= 2 and scratch == 0 and agpr == 0, t[kernel]
    assert lds <= 16 * 1024, lds  # the history slab: 64 rows x (3 n + 10) values
