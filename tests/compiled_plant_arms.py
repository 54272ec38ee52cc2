"""The built-in UR5's table as a compiled user arm, for the plant tests (tests/test_plant_gpu.py: the plugin's kernels are
the built-in's, bit for bit).  `__graft_entry__.build()` builds it into the in-tree plugin cache beside
tests/compiled_arms.py's; one hipcc run, skipped when the cached plugin matches the current kernel headers."""
from abr_control_amd import _abi, specialize


def table():
    tab = dict(_abi.load_table("ur5"))
    tab["name"] = "ur5_user"
    return tab


def build_all(verbose=False):
    abi = specialize.plugin_abi(from_sources=True)
    return {"ur5_user": specialize.compile_arm(table(), cache_dir=specialize.IN_TREE, abi=abi, verbose=verbose)}
