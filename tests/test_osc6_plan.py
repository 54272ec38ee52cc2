"""The launch form of the six-row law as a function of the batch size: `osc6_plan` (csrc/abrk_osc6_plan.h), evaluated
on the CPU through the hostsim test aid.  The table is what the library decided before the decision became one function
(it was spread over the host layer's scratch look-up, its three finish-parameter routines and two band rules in the
kernel header), quirks included; `rules_before` below is a literal transcription of those routines."""
import pytest

from tests import cases, hostsim

SHIPPED = dict(no_defer=0, no_handover=0, handover_max=65536, dense_max=1 << 20, finish_slots=0, finish_rounds=-1,
               finish_group=-1)


def rules_before(B, no_defer=0, no_handover=0, handover_max=65536, dense_max=1 << 20, finish_slots=0, finish_rounds=-1,
                 finish_group=-1):
    """-> (form, slots, rounds, group) as the routines named above chose them; slots / rounds / group are None where
    the launch did not read them"""
    k_block, k_handover_max_rows = 64, 262144
    nchunk = (B + k_block - 1) // k_block
    # the scratch look-up: worklist and / or records?
    wl = rec = False
    ho_max = handover_max if handover_max < k_handover_max_rows else k_handover_max_rows
    if not (no_defer or B > 0x7FFFFFFF):
        handover = (not no_handover) and B >= 64 and (B <= ho_max or B <= dense_max)
        if handover or B >= 16384:
            wl, rec = True, handover
    # the finish kernel's slots, rounds and group (-1: dense)
    slots = finish_slots if 1 <= finish_slots <= k_block else (12 if nchunk <= 256 else 8 if nchunk <= 512 else 2)
    rounds = min(finish_rounds, k_block) if finish_rounds >= 0 else (2 if nchunk <= 256 else 1)
    if B > ho_max:
        group = -1
    elif 0 <= finish_group <= 16:
        group = finish_group
    else:
        group = 16 if 128 < nchunk <= 256 else 0
    # what the launchers made of the pointers and of the sign of `group`
    if not wl:
        return "OnePass", None, None, None
    if not rec:
        return "Recompute", None, None, None
    if group < 0:
        return "HandoverDense", None, None, None
    if group > 0:
        return "HandoverGroup", slots, rounds, group
    return "HandoverChunk", slots, rounds, None


def agrees(plan, want):
    return plan[0] == want[0] and all(w is None or p == w for p, w in zip(plan[1:], want[1:]))


_ = None
TABLE = [
    # switches, B, form, slots, rounds, group
    ({}, 1, "OnePass", _, _, _),
    ({}, 63, "OnePass", _, _, _),
    ({}, 64, "HandoverChunk", 12, 2, _),
    ({}, 8192, "HandoverChunk", 12, 2, _),
    ({}, 8193, "HandoverGroup", 12, 2, 16),
    ({}, 16384, "HandoverGroup", 12, 2, 16),
    ({}, 16385, "HandoverChunk", 8, 1, _),
    ({}, 32768, "HandoverChunk", 8, 1, _),
    ({}, 32769, "HandoverChunk", 2, 1, _),
    ({}, 65536, "HandoverChunk", 2, 1, _),
    ({}, 65537, "HandoverDense", _, _, _),
    ({}, 1048576, "HandoverDense", _, _, _),
    ({}, 1048577, "Recompute", _, _, _),
    ({}, 2**31 - 1, "Recompute", _, _, _),
    ({}, 2**31, "OnePass", _, _, _),
    (dict(no_defer=1), 1, "OnePass", _, _, _),
    (dict(no_defer=1), 4096, "OnePass", _, _, _),
    (dict(no_defer=1), 300_037, "OnePass", _, _, _),
    (dict(no_defer=1), (1 << 20) + 12_325, "OnePass", _, _, _),
    (dict(no_handover=1), 16383, "OnePass", _, _, _),
    (dict(no_handover=1), 16384, "Recompute", _, _, _),
    (dict(no_handover=1), 300_037, "Recompute", _, _, _),
    (dict(dense_max=0), 65537, "Recompute", _, _, _),
    (dict(dense_max=4_000_000), 2_097_152, "HandoverDense", _, _, _),
    (dict(handover_max=262144), 262144, "HandoverChunk", 2, 1, _),
    (dict(handover_max=10**9), 262145, "HandoverDense", _, _, _),  # (the clamp)
    (dict(handover_max=1000), 5000, "HandoverDense", _, _, _),
    (dict(finish_group=0), 16384, "HandoverChunk", 12, 2, _),
    (dict(finish_group=3, finish_rounds=64), 4096, "HandoverGroup", 12, 64, 3),
    (dict(finish_rounds=0), 4096, "HandoverChunk", 12, 0, _),
    (dict(finish_slots=4, finish_rounds=200), 4096, "HandoverChunk", 4, 64, _),  # (rounds clamped)
    (dict(finish_slots=0), 4096, "HandoverChunk", 12, 2, _),  # (override ignored)
    (dict(finish_slots=65), 4096, "HandoverChunk", 12, 2, _),  # (override ignored)
]


@pytest.mark.parametrize("sw, B, form, slots, rounds, group", TABLE)
def test_osc6_plan_table(sw, B, form, slots, rounds, group):
    want = (form, slots, rounds, group)
    assert agrees(rules_before(B, **sw), want), (rules_before(B, **sw), want)  # (the table against the transcription)
    plan = hostsim.osc6_plan(B, **sw)
    assert agrees(plan, want), (plan, want)


SWEEP_SWITCHES = [{}, dict(no_defer=1), dict(no_handover=1), dict(dense_max=0), dict(dense_max=4_000_000),
                  dict(handover_max=262144), dict(handover_max=10**9), dict(handover_max=1000), dict(handover_max=-1),
                  dict(handover_max=0, dense_max=0), dict(finish_group=0), dict(finish_group=3, finish_rounds=64),
                  dict(finish_group=16), dict(finish_group=17), dict(finish_rounds=0), dict(finish_slots=4, finish_rounds=200),
                  dict(finish_slots=64), dict(finish_slots=65), dict(finish_slots=-3)]


@pytest.mark.parametrize("sw", SWEEP_SWITCHES, ids=lambda sw: ",".join(f"{k}={v}" for k, v in sw.items()) or "shipped")
def test_osc6_plan_equals_the_rules_it_replaced(sw):
    """every power of two from 1 to 2^32 and its neighbours, and the band edges in chunks"""
    sizes = {max(1, (1 << e) + d) for e in range(33) for d in (-1, 0, 1)}
    sizes |= {64 * c + d for c in (128, 256, 512, 1024, 4096) for d in (-64, -63, -1, 0, 1, 63, 64)}
    for B in sorted(sizes):
        plan, want = hostsim.osc6_plan(B, **sw), rules_before(B, **sw)
        assert agrees(plan, want), (B, sw, plan, want)


def test_osc6_plan_shipped_switches_are_the_defaults():
    for B in (1, 64, 16384, 65536, 65537, 1 << 20, (1 << 20) + 1):
        assert hostsim.osc6_plan(B) == hostsim.osc6_plan(B, **SHIPPED)


def test_gpu_suite_batch_sizes_take_the_forms_their_names_claim():
    """tests/cases.py GpuBackend and tests/test_gpu_six_row_large_batches.py pick batch sizes by form"""
    from tests import test_gpu_six_row_large_batches as big

    assert hostsim.osc6_plan(cases.GpuBackend.ONE_PASS_ROWS)[0] == "OnePass"
    assert hostsim.osc6_plan(cases.GpuBackend.DENSE_ROWS)[0] == "HandoverDense"
    assert hostsim.osc6_plan(cases.GpuBackend.RECOMPUTE_ROWS)[0] == "Recompute"
    assert (cases.GpuBackend.ONE_PASS_ROWS, cases.GpuBackend.DENSE_ROWS, cases.GpuBackend.RECOMPUTE_ROWS) == (
        48, 65536 + 128, (1 << 20) + 128)
    assert (big.GRID_ROWS, big.DENSE_TOP) == (4096 * 64, 1 << 20)
    assert hostsim.osc6_plan(big.DENSE_TOP)[0] == "HandoverDense"
    assert hostsim.osc6_plan(big.DENSE_TOP + 1)[0] == "Recompute"
    assert hostsim.osc6_plan(big.GRID_ROWS)[0] == hostsim.osc6_plan(big.GRID_ROWS + 1)[0] == "HandoverDense"
