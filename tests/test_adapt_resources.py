"""Register and LDS pin of the adaptive signal's kernels (no GPU needed: reads the gfx950 code object the build left in
abr_control_amd/csrc/build/, as tests/test_plant_resources.py does - skipped where there is no build).  The kernel is a
streaming pass over a row's state: nothing of it may spill (no scratch), it has no use for AGPRs, and its LDS is what
DESIGN.md "Adaptive signal" states - x_f (64 inputs), kappa e_f (16 outputs) and one reduction slot per wavefront and
output (4 x 16), in the kernel's type: 1152 bytes in fp64, 576 in fp32."""
import os

import pytest

from tests.test_kernel_resources import BUILD, _table

LDS = {"double": 1152, "float": 576}


@pytest.mark.skipif(not os.path.exists(os.path.join(BUILD, "abrk_adapt.o")), reason="no build in csrc/build")
def test_adapt_kernels_have_no_scratch_no_agprs_and_the_stated_lds():
    t = _table("abrk_adapt.o")
    seen = set()
    for name, (regs, agpr, waves, scratch, lds) in t.items():
        if "adapt_kernel<" not in name:
            continue
        args = name.split("adapt_kernel<")[1].split(">")[0].split(", ")
        ty, lif = args[0], args[1]
        seen.add((ty, lif))
        assert scratch == 0 and agpr == 0 and regs <= 256, (name, t[name])
        assert lds == LDS[ty], (name, lds)
    # fp64 / fp32 x lif / lif_rate (each in its 16-byte and its element-wise form)
    assert seen == {(ty, lif) for ty in ("double", "float") for lif in ("true", "false")}, sorted(t)
