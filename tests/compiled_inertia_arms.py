"""General-inertia user arms (full link inertias / joint inertias) whose compiled kernels the test-suite uses: the arm
tables of the reference fixtures tests/golden/inertia_<arm>.json (tools/gen_inertia_golden.py).
`__graft_entry__.build()` builds them into the in-tree plugin cache beside tests/compiled_arms.py's; one hipcc run each,
skipped when the cached plugin matches the current kernel headers."""
import json
import os
import threading

from abr_control_amd import specialize

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARMS = ("synthetic4", "ur5")


def table(arm):
    with open(os.path.join(GOLDEN, f"inertia_{arm}.json")) as fh:
        return json.load(fh)


def test_arms():
    return {arm: table(arm) for arm in ARMS}


def build_all(verbose=False):
    abi = specialize.plugin_abi(from_sources=True)
    out, err = {}, []

    def one(name, tab):
        try:
            out[name] = specialize.compile_arm(tab, cache_dir=specialize.IN_TREE, abi=abi, verbose=verbose)
        except Exception as e:  # noqa: BLE001 - re-raised on the caller's thread
            err.append(e)

    ths = [threading.Thread(target=one, args=kv) for kv in test_arms().items()]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    if err:
        raise err[0]
    return out
