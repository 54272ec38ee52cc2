"""Which kernel variant an OSC call runs: `osc_variant` (csrc/abrk_select.h), evaluated on the CPU through the hostsim
test aid.  The table is what the launcher decided before the decision became one function (it was spread over
`Launch::osc`, `osc_launch_feat`, `osc_launch`, `osc_full` and `osc_full_feat` of the kernel header, and copied by hand
into the test aid), quirks included; `rules_before` below is a literal transcription of those ladders."""
import itertools

import pytest

from abr_control_amd import _abi
from tests import hostsim

W_TX, W_C, W_DJ = _abi.WANT_TX, _abi.WANT_C, _abi.WANT_DJ


def rules_before(fast, n, use_C=False, n_null=0, tv=False, ki=0.0, ie=False, une=False, ts=True, want=0):
    """-> dict(km, use_c, feat, nots, full, vel) as the launcher's ladders chose the template arguments"""
    ie = ie and ki != 0  # (the host layer stages integrated_error for ki != 0 only)
    other = tv or ie or une
    if want:  # Launch::osc_full: the two-row kernel is not duplicated, x,y of a small arm takes the six-row form
        km = 3 if fast == 3 else 6
        # osc_full_feat
        plain = not other and n_null == 0
        if want & (W_C | W_DJ):
            feat, vel = 2, True
        elif plain:
            feat, vel = 0, False
        else:
            feat, vel = 2, False
        return dict(km=km, use_c=bool(use_C), feat=feat, nots=False, full=True, vel=vel)
    # Launch::osc
    if fast == 3:
        km = 3
    elif fast == 2 and n <= 3:
        km = 2
    else:
        km = 6
    # osc_launch_feat: 0 none, 1 fused null controllers only, 2 anything else
    feat = 2 if other else 1 if n_null > 0 else 0
    # osc_launch
    nots = km == 6 and feat == 0 and not ts
    return dict(km=km, use_c=bool(use_C), feat=feat, nots=nots, full=False, vel=False)


def V(km, feat, use_c=False, nots=False, full=False, vel=False):
    return dict(km=km, use_c=use_c, feat=feat, nots=nots, full=full, vel=vel)


TABLE = {
    # name: (fast, n, call, variant)
    "xyz": (3, 6, {}, V(3, 0)),
    "xyz_no_training_signal": (3, 6, dict(ts=False), V(3, 0)),
    "xyz_use_C": (3, 6, dict(use_C=True), V(3, 0, use_c=True)),
    "xy_twojoint": (2, 2, {}, V(2, 0)),
    "xy_threejoint_use_C": (2, 3, dict(use_C=True), V(2, 0, use_c=True)),
    "xy_fourjoint": (2, 4, {}, V(6, 0)),  # (no two-row kernel beyond three joints)
    "xy_fourjoint_no_training_signal": (2, 4, dict(ts=False), V(6, 0, nots=True)),
    "six_row": (0, 6, {}, V(6, 0)),
    "six_row_no_training_signal": (0, 6, dict(ts=False), V(6, 0, nots=True)),
    "six_row_use_C_no_training_signal": (0, 7, dict(use_C=True, ts=False), V(6, 0, use_c=True, nots=True)),
    "nulls_only_xyz": (3, 6, dict(n_null=2), V(3, 1)),
    "nulls_only_six_row": (0, 6, dict(n_null=1, ts=False), V(6, 1)),  # (NOTS: the plain law alone)
    "target_velocity": (3, 6, dict(tv=True), V(3, 2)),
    "u_null_ext": (0, 6, dict(une=True, ts=False), V(6, 2)),
    "target_velocity_and_nulls": (3, 6, dict(tv=True, n_null=1), V(3, 2)),
    "ki_with_state": (3, 6, dict(ki=0.2, ie=True), V(3, 2)),
    "ki_zero_with_state": (3, 6, dict(ki=0.0, ie=True), V(3, 0)),  # (the state array is not staged)
    "ki_zero_with_state_six_row": (0, 6, dict(ki=0.0, ie=True, ts=False), V(6, 0, nots=True)),
    "ki_without_state": (3, 6, dict(ki=0.2), V(3, 0)),  # (the host layer refuses the call before it gets here)
    "full_Tx_plain": (3, 6, dict(want=W_TX), V(3, 0, full=True)),
    "full_Tx_plain_use_C": (3, 6, dict(want=W_TX, use_C=True), V(3, 0, use_c=True, full=True)),
    "full_Tx_nulls": (3, 6, dict(want=W_TX, n_null=1), V(3, 2, full=True)),  # (the fused FEAT is 0 or 2)
    "full_Tx_target_velocity": (0, 6, dict(want=W_TX, tv=True), V(6, 2, full=True)),
    "full_Tx_xy_twojoint": (2, 2, dict(want=W_TX), V(6, 0, full=True)),  # (the fused kernel has no two-row form)
    "full_Tx_no_training_signal": (0, 6, dict(want=W_TX, ts=False), V(6, 0, full=True)),  # (and no NOTS form)
    "full_C_plain": (3, 6, dict(want=W_C), V(3, 2, full=True, vel=True)),  # (VEL forces FEAT 2)
    "full_dJ_plain": (0, 6, dict(want=W_DJ | W_TX), V(6, 2, full=True, vel=True)),
    "full_C_nulls": (3, 6, dict(want=W_C | W_TX, n_null=2, use_C=True), V(3, 2, use_c=True, full=True, vel=True)),
    "full_dJ_u_null_ext": (0, 6, dict(want=W_DJ, une=True), V(6, 2, full=True, vel=True)),
}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_osc_variant_table(name):
    fast, n, call, want = TABLE[name]
    assert rules_before(fast, n, **call) == want  # (the table against the transcription)
    assert hostsim.osc_variant(fast, n, **call) == want


def test_osc_variant_equals_the_rules_it_replaced():
    """every combination of what a call can present, for every `fast`, arms on both sides of the two-row kernel's
    three-joint limit, the law alone and the fused kernel with and without velocity-dependent outputs"""
    flags = ("use_C", "nulls", "tv", "ki", "ie", "une", "ts")
    count = 0
    for bits in itertools.product((False, True), repeat=len(flags)):
        f = dict(zip(flags, bits))
        call = dict(use_C=f["use_C"], n_null=2 if f["nulls"] else 0, tv=f["tv"], ki=0.2 if f["ki"] else 0.0,
                    ie=f["ie"], une=f["une"], ts=f["ts"])
        for fast, n, want in itertools.product((0, 2, 3), (2, 3, 6), (0, W_TX, W_C)):
            got, ref = hostsim.osc_variant(fast, n, want=want, **call), rules_before(fast, n, want=want, **call)
            assert got == ref, (fast, n, want, call, got, ref)
            count += 1
    assert count == 2 ** 7 * 27


def test_want_bits_are_the_ones_the_rule_reads():
    """abrk_select.h names the velocity-dependent outputs by their bits (the kernel header asserts the same against W_C | W_DJ)"""
    assert (W_C, W_DJ) == (1 << 4, 1 << 5)
    for want, vel in ((W_TX, False), (W_C, True), (W_DJ, True), (_abi.WANT_J | _abi.WANT_M | _abi.WANT_G, False)):
        assert hostsim.osc_variant(3, 6, want=want)["vel"] == vel
