"""Register and LDS pin of the measurement channel's kernels (no GPU needed: reads the gfx950 code object the build left
in abr_control_amd/csrc/build/, as tests/test_adapt_resources.py does - skipped where there is no build).  One lane per
element: nothing of it may spill (no scratch), it has no use for AGPRs or LDS, and there are four
instantiations - fp64 and fp32, each with the generator and, for a launch in which every sigma is zero, without."""
import os

import pytest

from tests.test_kernel_resources import BUILD, _table


@pytest.mark.skipif(not os.path.exists(os.path.join(BUILD, "abrk_channel.o")), reason="no build in csrc/build")
def test_channel_kernels_have_no_scratch_no_agprs_and_no_lds():
    t = _table("abrk_channel.o")
    seen = {}
    for name, (regs, agpr, waves, scratch, lds) in t.items():
        if "channel_kernel<" not in name:
            continue
        ty, noise = name.split("channel_kernel<")[1].split(">")[0].split(", ")
        seen[(ty, noise)] = regs
        assert scratch == 0 and agpr == 0 and lds == 0, (name, t[name])
        assert regs <= 128 and waves >= 4, (name, t[name])  # at least four wavefronts per SIMD with the generator's log and cos
    assert set(seen) == {(ty, noise) for ty in ("double", "float") for noise in ("true", "false")}, sorted(t)
    # the instantiation without the generator is the small one
    for ty in ("double", "float"):
        assert seen[(ty, "false")] < seen[(ty, "true")] and seen[(ty, "false")] <= 64, seen
