"""Resource pin of the force-control kernel (no GPU needed: reads the gfx950 code objects the build left in
abr_control_amd/csrc/build/, as tests/test_contact_resources.py does - skipped where there is no build).  The row is one
dynamics pass without Coriolis terms, the point Jacobian, a Cholesky factor of M and the 3 x 3 task-space inertia: on a
compile-time table it holds two wavefronts per SIMD without scratch, accumulator registers or LDS in both dtypes; the
fp64 row of a runtime table takes the registers it needs at one wavefront per SIMD, without scratch either
(profiles/force_control.md has the table; the waves per SIMD are recorded there, not promised here).  The kernels
beside it keep the budgets their own tests pin."""
import os

import pytest

from tests.test_kernel_resources import BUILD, _table

UR5 = "abrk::StaticArm<abrk::Tab_ur5>"


def _need(obj):
    if not os.path.exists(os.path.join(BUILD, obj)):
        pytest.skip("no build in csrc/build")
    return _table(obj)


def test_ur5_force_kernels_have_no_scratch_inside_256_registers():
    t = _need("abrk_arm_ur5.o")
    for T in ("double", "float"):
        k = f"force_kernel<{UR5}, {T}>"
        assert k in t, f"{k} not found in abrk_arm_ur5.o"
        regs, agpr, waves, scratch, lds = t[k]
        assert scratch == 0 and agpr == 0 and regs <= 256, (k, t[k])
        assert lds == 0, (k, lds)


@pytest.mark.parametrize("obj", ("abrk_arm_jaco2.o", "abrk_arm_rt6.o"))
def test_the_force_kernel_is_instantiated_for_general_chains_and_runtime_tables(obj):
    t = _need(obj)
    ks = sorted(k for k in t if k.startswith("force_kernel<"))
    assert len(ks) == 2 and any(k.endswith("double>") for k in ks) and any(k.endswith("float>") for k in ks), (obj, ks)
    for k in ks:
        assert t[k][3] == 0 and t[k][4] == 0, (k, t[k])  # no scratch, no LDS


def test_the_kernels_beside_it_keep_their_budgets():
    """what tests/test_contact_resources.py, test_plant_payload_resources.py and test_loop_trace_resources.py pin, on
    the same objects"""
    t = _need("abrk_arm_ur5.o")
    regs, agpr, waves, scratch, lds = t[f"contact_kernel<{UR5}, double>"]
    assert scratch == 0 and agpr == 0 and waves >= 2 and regs <= 256 and lds == 0
    regs, agpr, waves, scratch, lds = t[f"plant_fx_kernel<{UR5}, double>"]
    assert scratch == 0 and agpr == 0 and regs <= 256 and waves >= 2 and lds <= 24 * 1024
    regs, agpr, waves, scratch, lds = t[f"plant_kernel<{UR5}, double>"]
    assert scratch == 0 and agpr == 0 and regs <= 256 and waves >= 2 and lds <= 20 * 1024
    regs, agpr, waves, scratch, lds = t[f"trace_kernel<{UR5}, double>"]
    assert waves >= 2 and scratch == 0 and agpr == 0 and lds <= 16 * 1024
