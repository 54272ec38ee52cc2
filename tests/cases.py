"""The parity cases shared by every backend (oracle, hostsim, GPU).

Each controller case names the golden arrays written by oracle/gen_golden.py (outputs of
the REFERENCE itself: `<key>_uS` as shipped, `<key>_uD` same formulas in fp64) and how
to rebuild the same controller through the C-ABI parameter structs.
"""
import numpy as np

from abr_control_amd import _abi
from abr_control_amd._abi import (make_damping, make_joint, make_osc_params as P, make_resting,
                                  make_sliding_params as SP)

XYZ = [1, 1, 1, 0, 0, 0]
SIX = [1] * 6
XY = [1, 1, 0, 0, 0, 0]

# key -> (arm, kind, builder(n) -> kwargs)
CASES = {}


def _osc(arm, key, params, tv=False, steps=1):
    CASES[f"{arm}:{key}"] = dict(arm=arm, key=key, kind="osc", params=params, tv=tv, steps=steps)


def _sl(arm, key, params, tvf=None, taf=None):
    CASES[f"{arm}:{key}"] = dict(arm=arm, key=key, kind="sliding", params=params, tvf=tvf, taf=taf)


def _jt(arm, key, ctrl, grav, tscale=1.0, tvf=None, no_target=False):
    CASES[f"{arm}:{key}"] = dict(arm=arm, key=key, kind="joint", ctrl=ctrl, grav=grav, tscale=tscale, tvf=tvf,
                                 no_target=no_target)


# ---- twojoint (BASELINE config 1 = cfg1)
_osc("twojoint", "cfg1", lambda n: P(n, kp=10, kv=3, ctrlr_dof=XY))
_osc("twojoint", "osc_xy_vmax", lambda n: P(n, kp=20, kv=5, ctrlr_dof=XY, vmax=[0.5, 0.5]))
_osc("twojoint", "osc_xy_C", lambda n: P(n, kp=10, kv=3, ctrlr_dof=XY, use_C=True))
_sl("twojoint", "sliding", lambda n: SP(n))
# ---- onejoint (N_LINKS = 1: M, g, C vanish identically - only the controllers that never invert M run in the reference)
_sl("onejoint", "sliding", lambda n: SP(n))
_sl("onejoint", "sliding_tv", lambda n: SP(n, kd=20.0, lamb=5.0), tvf=lambda t: t[:, ::-1] * 0.3, taf=lambda t: t * 0.1)
# ---- threejoint (BASELINE config 5 = cfg5)
_sl("threejoint", "cfg5", lambda n: SP(n))
_sl("threejoint", "sliding_tv", lambda n: SP(n, kd=20.0, lamb=5.0), tvf=lambda t: t[:, ::-1] * 0.3,
    taf=lambda t: t * 0.1)
_osc("threejoint", "osc_xy", lambda n: P(n, kp=50, ctrlr_dof=XY))
for _alg in (0, 1):
    _osc("threejoint", f"osc_xyg_alg{_alg}",
         lambda n, a=_alg: P(n, kp=50, ko=20, kv=8, ctrlr_dof=[1, 1, 0, 0, 0, 1], orientation_algorithm=a))
_jt("threejoint", "joint", make_joint(20, 4), True)
# ---- ur5 (BASELINE configs 2 and 4)
_osc("ur5", "cfg2", lambda n: P(n, kp=200, ctrlr_dof=XYZ))
_osc("ur5", "cfg4", lambda n: P(n, kp=200, ctrlr_dof=XYZ, use_g=True, use_C=True))
for _alg in (0, 1):
    _osc("ur5", f"osc6_alg{_alg}",
         lambda n, a=_alg: P(n, kp=200, ko=150, kv=25, ctrlr_dof=SIX, orientation_algorithm=a))
_osc("ur5", "osc_xyz_vmax_ki", lambda n: P(n, kp=100, kv=15, ki=0.2, ctrlr_dof=XYZ, vmax=[0.5, 1.0]), steps=5)
_osc("ur5", "osc6_vmax", lambda n: P(n, kp=100, ko=80, kv=15, ctrlr_dof=SIX, vmax=[0.5, 1.0]))
_osc("ur5", "osc_xyz_tvel", lambda n: P(n, kp=200, ctrlr_dof=XYZ), tv=True)
_osc("ur5", "osc_nog", lambda n: P(n, kp=30, kv=7, ctrlr_dof=XYZ, use_g=False))
_osc("ur5", "osc_offset", lambda n: P(n, kp=200, ctrlr_dof=XYZ, xyz_offset=[0.11, -0.23, 0.37]))
_osc("ur5", "osc_link5", lambda n: P(n, kp=200, ctrlr_dof=XYZ, ref_frame="link5"))
_osc("ur5", "osc_abg", lambda n: P(n, kp=100, ko=60, kv=12, ctrlr_dof=[0, 0, 0, 1, 1, 1]))
_osc("ur5", "osc_xz_b", lambda n: P(n, kp=100, ko=60, kv=12, ctrlr_dof=[1, 0, 1, 0, 1, 0]))
_osc("ur5", "osc_null2", lambda n: P(n, kp=200, ctrlr_dof=XYZ, null_controllers=[
    make_damping(10), make_resting([None, 0.8, -1.6, None, 1.5, None], kp=40, kv=8)]))
_jt("ur5", "joint", make_joint(50, 9), True, tscale=3.0)
_jt("ur5", "joint_tv_nog", make_joint(50), False, tscale=3.0, tvf=lambda t: t[:, ::-1])
_sl("ur5", "sliding", lambda n: SP(n))
# ---- jaco2 (BASELINE config 3)
_osc("jaco2", "cfg3", lambda n: P(n, kp=200, ctrlr_dof=XYZ, null_controllers=[make_damping(10)]))
_osc("jaco2", "osc5", lambda n: P(n, kp=200, ctrlr_dof=[1] * 5 + [0]))
_osc("jaco2", "osc6_alg1", lambda n: P(n, kp=200, ko=150, kv=25, ctrlr_dof=SIX, orientation_algorithm=1))
_osc("jaco2", "osc_rest", lambda n: P(n, kp=200, ctrlr_dof=XYZ, null_controllers=[
    make_resting([None, 3.14, 1.57, None, None, 3.04], kp=30, kv=6)]))
_jt("jaco2", "damping", make_damping(10), False, no_target=True)


def takes_plain_six_row_law(case_id):
    """True where the case runs the six-row kernels with no optional input (`osc_kernel<.., 6, .., FEAT = 0, ..>`: not the
    x,y,z / x,y fast paths of abrk_params.h osc_fast_rows, no target velocity, no integral state, no fused secondary
    controller) - the law that has a `NOTS = true` twin for callers who ask for no training signal.  The launcher's own
    rule answers (csrc/abrk_select.h `osc_variant`, through the hostsim test aid)"""
    from tests import hostsim

    case = CASES[case_id]
    if case["kind"] != "osc":
        return False
    n = _abi.load_table(case["arm"])["n_joints"]
    p = case["params"](n)
    dof = [int(bool(v)) for v in p.ctrlr_dof]
    ee = p.ref_frame == 2 * n + 1
    fast = 0 if not ee else 3 if dof == XYZ else 2 if dof == XY and n <= 3 else 0
    v = hostsim.osc_variant(fast, n, use_C=p.use_C, n_null=p.n_null, tv=case["tv"], ki=p.ki, ie=case["steps"] > 1)
    return v["km"] == 6 and v["feat"] == 0


def run_case(backend, case, g, dtype=np.float64, rows=None):
    """Evaluate one case on a backend.  Returns (u, extra) with u shaped like `<key>_uD`."""
    key = case["key"]
    n = backend.n
    sl = slice(None) if rows is None else slice(0, rows)
    q, dq, t = g[f"{key}_q"][sl], g[f"{key}_dq"][sl], g[f"{key}_target"][sl]
    if case["kind"] == "osc":
        params = case["params"](n)
        tv = g[f"{key}_tvel"][sl] if case["tv"] else None
        if case["steps"] == 1:
            u, ts = backend.osc(params, q, dq, t, tv, dtype=dtype)
            return u, dict(ts=ts)
        ie = np.zeros((len(q), 6), dtype)
        us = []
        for _ in range(case["steps"]):  # same inputs each step: only integrated_error evolves
            u, _ts = backend.osc(params, q, dq, t, tv, ie=ie, dtype=dtype)
            us.append(u)
        return np.array(us), {}
    if case["kind"] == "sliding":
        tv = case["tvf"](t) if case["tvf"] else None
        ta = case["taf"](t) if case["taf"] else None
        u, s = backend.sliding(case["params"](n), q, dq, t, tv, ta, dtype=dtype)
        return u, dict(s=s)
    tt = None if case["no_target"] else t * case["tscale"]
    tv = case["tvf"](t) if case["tvf"] else None
    return backend.joint(case["ctrl"], case["grav"], q, dq, tt, tv, dtype=dtype), {}


def rel_err(a, b):
    """max|a-b| / max|b| per row (the metric of BASELINE.md / SURVEY.md section 8c)"""
    return np.max(np.abs(a - b), axis=-1) / np.max(np.abs(b), axis=-1)


def threshold_band(g, key, eps=1e-6):
    """rows whose Mx_inv sits within `eps` (relative) of either `_Mx` threshold (osc.py:138,145):
    |det| ~ 1e-3, or a singular value ~ 1e-4 * max while |det| < 1e-3.  Their output may
    legitimately flip between the inv and the truncated-pinv answer under rounding."""
    if f"{key}_det" not in g:
        return None
    det, sv = np.abs(g[f"{key}_det"]), g[f"{key}_sv"]
    near_det = np.abs(det - 1e-3) <= eps * 1e-3
    with np.errstate(invalid="ignore", divide="ignore"):  # an all-zero Mx_inv (a row without task rows) has no band
        ratio = sv / sv.max(axis=1, keepdims=True)
    near_cut = (np.abs(ratio - 1e-4) <= eps * 1e-4).any(axis=1) & (det < 1e-3 * (1 + eps))
    return near_det | near_cut


def truncating_rows(g, key):
    """rows on which `pinv(Mx_inv, rcond=1e-4)` really drops a singular value (osc.py:142-145): |det| < 1e-3 and
    min(sv) < 1e-4 max(sv).  These rows are NOT excluded from the golden assert (only the 1e-6-relative band
    around the two thresholds is) - the count is reported so that a test can insist they were compared."""
    if f"{key}_det" not in g:
        return None
    det, sv = np.abs(g[f"{key}_det"]), g[f"{key}_sv"]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = sv / sv.max(axis=1, keepdims=True)
    return (det < 1e-3) & (ratio.min(axis=1) < 1e-4)


def mx_rows_clear_of_thresholds(det, sv, eps=1e-6):
    """the same band test for `_Mx` called directly (fixtures oschelpers_<arm>.npz): True = safe to compare"""
    det, sv = np.abs(np.asarray(det)), np.asarray(sv)
    near_det = np.abs(det - 1e-3) <= eps * 1e-3
    with np.errstate(invalid="ignore", divide="ignore"):  # an all-zero Mx_inv (a row without task rows) has no band
        ratio = sv / sv.max(axis=1, keepdims=True)
    near_cut = (np.abs(ratio - 1e-4) <= eps * 1e-4).any(axis=1) & (det < 1e-3 * (1 + eps))
    return ~(near_det | near_cut)


# ---------------------------------------------------------------------------- backends
class OracleBackend:
    name = "oracle"

    def __init__(self, arm):
        from oracle.oracle import Oracle

        self.o = Oracle(_abi.load_table(arm))
        self.n = self.o.n

    def osc(self, params, q, dq, t, tv=None, ie=None, une=None, dtype=np.float64):
        return self.o.osc_batch(params, q, dq, t, tv, ie, une, want_training=True)

    def sliding(self, params, q, dq, t, tv=None, ta=None, dtype=np.float64):
        return self.o.sliding_batch(params, q, dq, t, tv, ta)

    def joint(self, ctrl, grav, q, dq, t=None, tv=None, dtype=np.float64):
        return self.o.joint_batch(ctrl, grav, q, dq, t, tv)

    def limits(self, params, q, dtype=np.float64):
        from oracle.oracle import avoid_joint_limits_batch

        return avoid_joint_limits_batch(self.n, params, q)

    def floating(self, dynamic, task_space, q, dq, dtype=np.float64):
        return self.o.floating_batch(dynamic, task_space, q, dq)[0]

    def obstacles(self, params, q, dtype=np.float64):
        return self.o.avoid_obstacles_batch(params, q)[0]

    def dynamics(self, q, dq=None, frame="EE", x_off=None, want=("M",), dtype=np.float64):
        o, B = self.o, len(q)
        f = {"Tx": lambda i: o.Tx(frame, q[i], x_off), "J": lambda i: o.J(frame, q[i], x_off),
             "M": lambda i: o.M(q[i]), "g": lambda i: o.g(q[i]), "C": lambda i: o.C(q[i], dq[i]),
             "dJ": lambda i: o.dJ(frame, q[i], dq[i], x_off), "R": lambda i: o.R(frame, q[i]),
             "T": lambda i: o.T(frame, q[i]), "Tinv": lambda i: o.T_inv(frame, q[i]),
             "quat": lambda i: o.quaternion(frame, q[i])}
        return {w: np.array([f[w](i) for i in range(B)]) for w in want}


class HostsimBackend:
    """the GPU row programs compiled for the CPU (tests/hostsim) - static or runtime-table arm"""

    def __init__(self, arm, variant="static", handover=False, training_signal=True):
        """handover: six-row laws run in the two-pass form libabrk launches up to 262144 rows (first pass without the
        eigen-decomposition, deferred rows finished from their hand-over records); `deferred` counts those rows.
        training_signal=False: the call asks for no training signal, as bench.py and any C-ABI caller without that
        buffer do - the plain six-row law then runs its NoTs arithmetic (osc() returns (u, None))"""
        from tests import hostsim

        self.h = hostsim
        if isinstance(arm, dict):  # a user arm table -> runtime-table row programs
            self.tab, variant = arm, "rt"
        else:
            self.tab = _abi.load_table(arm)
        self.n = self.tab["n_joints"]
        self.arm = arm if variant == "static" else self.tab
        self.name = f"hostsim-{variant}" + ("-handover" if handover else "") + ("" if training_signal else "-nots")
        self.handover = handover
        self.training_signal = training_signal
        self.deferred = 0

    def osc(self, params, q, dq, t, tv=None, ie=None, une=None, dtype=np.float64):
        want = bool(self.training_signal)
        if self.handover:
            r = self.h.osc_generate(self.arm, params, q, dq, t, tv, ie, une, training_signal=want, dtype=dtype,
                                    handover=True)
            self.deferred += max(r[-1], 0)
            return (r[0], r[1]) if want else (r[0], None)
        r = self.h.osc_generate(self.arm, params, q, dq, t, tv, ie, une, training_signal=want, dtype=dtype)
        return r if want else (r, None)

    def sliding(self, params, q, dq, t, tv=None, ta=None, dtype=np.float64):
        return self.h.sliding_generate(self.arm, params, q, dq, t, tv, ta, want_s=True, dtype=dtype)

    def joint(self, ctrl, grav, q, dq, t=None, tv=None, dtype=np.float64):
        return self.h.joint_generate(self.arm, ctrl, grav, q, dq, t, tv, dtype=dtype)

    def limits(self, params, q, dtype=np.float64):
        return self.h.avoid_joint_limits_generate(self.n, params, q, dtype=dtype)

    def floating(self, dynamic, task_space, q, dq, dtype=np.float64):
        return self.h.floating_generate(self.arm, dynamic, task_space, q, dq, dtype=dtype)

    def obstacles(self, params, q, dtype=np.float64):
        return self.h.avoid_obstacles_generate(self.arm, params, q, dtype=dtype)

    def dynamics(self, q, dq=None, frame="EE", x_off=None, want=("M",), dtype=np.float64):
        return self.h.dynamics(self.arm, q, dq, _abi.frame_id(frame, self.n), x_off, want, dtype)


class GpuBackend:
    """libabrk.so through the C ABI (abr_control_amd.engine) - static or runtime-table arm"""

    # rows per call of the forms of the six-row law (csrc/abrk_osc6_plan.h osc6_plan; tests/test_osc6_plan.py checks that
    # these sizes take the forms their names claim: one pass below one
    # wavefront of rows; hand-over records + per-chunk or grouped finish kernel up to 65 536 rows; hand-over records + the
    # dense finish kernel up to 1 048 576 rows; worklist + recompute pass beyond)
    ONE_PASS_ROWS, DENSE_ROWS, RECOMPUTE_ROWS = 48, 65536 + 128, (1 << 20) + 128

    def __init__(self, arm, variant="static", device=0, training_signal=True, form="auto"):
        """training_signal=False: ask for no training signal - what bench.py times and what a C-ABI caller without that
        buffer gets (the plain six-row law then runs the `NOTS = true` instantiations); osc() returns (u, None).
        form: "auto" = one call on the rows as given; "slices" = calls of ONE_PASS_ROWS rows (the six-row law in one
        pass: `osc_kernel<.., PASS = 0>` in mode 0); "tiled" = the rows repeated up to DENSE_ROWS (first pass on hand-over
        records, `PASS = 1` in mode 1, then the dense finish kernel, abrk_finish.h osc6_finish_dense_kernel); "recompute" =
        the rows repeated up to RECOMPUTE_ROWS, beyond 1 M (first pass + recompute pass over the worklist: `PASS = 1` in
        mode 1, then `PASS = 0` in mode 2).  Tiled forms: every repetition bit-equal."""
        import ctypes as C

        from abr_control_amd import engine
        from abr_control_amd._lib import check, lib

        self.e = engine
        if isinstance(arm, dict):  # a user arm table -> runtime-table kernels ("compiled": its plugin, specialize.py)
            self.tab, variant = arm, ("compiled" if variant == "compiled" else "rt")
        else:
            self.tab = _abi.load_table(arm)
        self.n = self.tab["n_joints"]
        self.device = device
        if variant == "static":
            self.arm_id = check(lib().abrk_arm_builtin(arm.encode()))
        elif variant == "compiled":
            from abr_control_amd import specialize

            path = specialize.find_compiled(self.tab)
            assert path, "no compiled plugin for this arm and the current kernel headers: run __graft_entry__.build()"
            d = _abi.desc_from_table(self.tab)
            self.arm_id = check(lib().abrk_arm_create_compiled(C.byref(d), path.encode()))
        else:
            d = _abi.desc_from_table(self.tab)
            self.arm_id = check(lib().abrk_arm_create(C.byref(d)))
        self.training_signal, self.form = training_signal, form
        self.name = f"gpu-{variant}" + ("" if training_signal else "-nots") + ("" if form == "auto" else f"-{form}")
        self._owned = variant != "static"

    def __del__(self):  # user arms are registered per backend: hand the slot back (fuzz runs create thousands)
        try:
            if self._owned:
                from abr_control_amd._lib import lib

                lib().abrk_arm_destroy(self.arm_id)
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def _osc(self, params, q, dq, t, tv, ie, une, dtype):
        want = bool(self.training_signal)
        r = self.e.osc_generate(self.arm_id, self.n, params, q, dq, t, tv, ie, une, training_signal=want,
                                dtype=dtype, device=self.device)
        return r if want else (r, None)

    def osc(self, params, q, dq, t, tv=None, ie=None, une=None, dtype=np.float64):
        if self.form == "auto":
            return self._osc(params, q, dq, t, tv, ie, une, dtype)
        B = len(q)
        cut = lambda a, lo, hi: None if a is None else a[lo:hi]  # row slices of C-contiguous arrays: views, in place
        if self.form == "slices":
            parts = [self._osc(params, q[lo:lo + self.ONE_PASS_ROWS], dq[lo:lo + self.ONE_PASS_ROWS],
                               t[lo:lo + self.ONE_PASS_ROWS], cut(tv, lo, lo + self.ONE_PASS_ROWS),
                               cut(ie, lo, lo + self.ONE_PASS_ROWS), cut(une, lo, lo + self.ONE_PASS_ROWS), dtype)
                     for lo in range(0, B, self.ONE_PASS_ROWS)]
            u = np.concatenate([p[0] for p in parts])
            return u, (np.concatenate([p[1] for p in parts]) if self.training_signal else None)
        assert self.form in ("tiled", "recompute"), self.form
        reps = -(-(self.DENSE_ROWS if self.form == "tiled" else self.RECOMPUTE_ROWS) // B)
        rep = lambda a: None if a is None else np.ascontiguousarray(np.tile(np.asarray(a), (reps, 1)))
        ie_t = rep(ie)
        u, ts = self._osc(params, rep(q), rep(dq), rep(t), rep(tv), ie_t, rep(une), dtype)
        for k in range(1, reps):  # a row's bits do not depend on where in the batch it sits
            assert np.array_equal(u[k * B:(k + 1) * B], u[:B], equal_nan=True), f"{self.name}: repetition {k} differs"
        if ie is not None:
            ie[...] = ie_t[:B]
        return np.ascontiguousarray(u[:B]), (None if ts is None else np.ascontiguousarray(ts[:B]))

    def sliding(self, params, q, dq, t, tv=None, ta=None, dtype=np.float64):
        return self.e.sliding_generate(self.arm_id, self.n, params, q, dq, t, tv, ta, want_s=True, dtype=dtype,
                                       device=self.device)

    def joint(self, ctrl, grav, q, dq, t=None, tv=None, dtype=np.float64):
        return self.e.joint_generate(self.arm_id, self.n, ctrl, grav, q, dq, t, tv, dtype=dtype, device=self.device)

    def limits(self, params, q, dtype=np.float64):
        return self.e.avoid_joint_limits_generate(self.n, params, np.asarray(q), dtype=dtype, device=self.device)

    def floating(self, dynamic, task_space, q, dq, dtype=np.float64):
        return self.e.floating_generate(self.arm_id, self.n, dynamic, task_space, np.asarray(q), dq, dtype=dtype,
                                        device=self.device)

    def obstacles(self, params, q, dtype=np.float64):
        return self.e.avoid_obstacles_generate(self.arm_id, self.n, params, np.asarray(q), dtype=dtype,
                                               device=self.device)

    def dynamics(self, q, dq=None, frame="EE", x_off=None, want=("M",), dtype=np.float64):
        return self.e.dynamics(self.arm_id, self.n, np.asarray(q), dq, _abi.frame_id(frame, self.n), x_off, want,
                               dtype, self.device)


# ---------------------------------------------------------------------------- shared assertions
# Tolerances (documented in DESIGN.md):
#   fp64 vs Oracle-D (reference formulas in fp64): 1e-6 relative, the north_star bound.  Observed ~1e-13.
#   threejoint: the reference's own functions disagree with each other at ~1e-7 because its link
#     lengths are float32 and SymPy folds them at 24-bit precision (threejoint/config.py:52-67).
#   fp32 kernels (config 5): 1e-4 relative vs the as-shipped reference, BASELINE.json configs[4].
TOL_D = 1e-6
TOL_F32 = 1e-4
TOL_THREEJOINT = 2e-5  # the reference's own float32-`L` inconsistency (see above), amplified by pinv
# (median, p99) caps of max|du|/max|u| against the as-shipped (float32-rounding) reference path on the BASELINE configs;
# the reference's own fp64 formulas sit at median 0.8-1.4e-7, p99 0.5-2.4e-6 from it (cfg1: p99 1.2e-5, truncated pinv)
SHIPPED_CAPS = {"ur5:cfg2": (2e-7, 5e-6), "ur5:cfg4": (2e-7, 5e-6), "jaco2:cfg3": (2e-7, 5e-6),
                "threejoint:cfg5": (2e-7, 5e-6), "twojoint:cfg1": (2e-7, 5e-5)}


def check_case_against_golden(backend, case_id, g, dtype=np.float64, rows=None):
    case = CASES[case_id]
    key = case["key"]
    u, extra = run_case(backend, case, g, dtype, rows)
    sl = slice(None) if rows is None else slice(0, rows)
    uD, uS = g[f"{key}_uD"], g[f"{key}_uS"]
    if case.get("steps", 1) > 1:
        uD, uS = uD[:, sl], uS[:, sl]
    else:
        uD, uS = uD[sl], uS[sl]
    assert u.shape == uD.shape
    assert np.all(np.isfinite(u)), f"{case_id}: non-finite output"
    rD = rel_err(np.asarray(u, dtype=float), uD)
    band = threshold_band(g, key)
    ok = np.ones(rD.shape, bool)
    if band is not None:
        ok &= ~band[sl]
    tol = TOL_D if dtype == np.float64 else TOL_F32
    if case["arm"] == "threejoint" and dtype == np.float64:
        tol = TOL_THREEJOINT
    if dtype != np.float64:
        # fp32 arithmetic: conditioning of Mx_inv amplifies rounding; keep well-conditioned rows.  Three task rows:
        # cond < 1e3.  Six rows mix metres and radians - cond(Mx_inv) starts at ~1e3 - so the gate is 1e4 there (observed
        # error <= 1.6e-8 cond on the golden sets), and every row up to cond 1e6 that does not truncate is held to
        # 1e-7 cond on top, so that the ill-conditioned rows are not simply dropped.
        if f"{key}_sv" in g:
            sv = g[f"{key}_sv"][sl]
            cond = sv.max(1) / np.maximum(sv.min(1), 1e-300)
            six = sv.shape[1] > 3
            if six:
                trunc32 = truncating_rows(g, key)[sl]
                wide = ok & (cond < 1e6) & ~trunc32
                assert wide.sum() >= 0.5 * len(cond), f"{case_id}: only {wide.sum()} of {len(cond)} rows compared"
                bad = rD[wide] > np.maximum(tol, 1e-7 * cond[wide])
                assert not bad.any(), f"{case_id} [{backend.name}]: fp32 error above 1e-7 cond on {bad.sum()} rows"
            ok &= cond < (1e4 if six else 1e3)
            assert ok.sum() >= 0.25 * len(cond), f"{case_id}: only {ok.sum()} of {len(cond)} well-conditioned rows"
    worst = rD[ok].max() if ok.any() else 0.0
    assert worst <= tol, f"{case_id} [{backend.name}]: max rel err vs Oracle-D {worst:.3e} > {tol}"
    if "ts" in extra and extra["ts"] is not None and f"{key}_tsD" in g and dtype == np.float64:
        rT = rel_err(np.asarray(extra["ts"], float), g[f"{key}_tsD"][sl])
        assert rT[ok].max() <= tol, f"{case_id}: training_signal {rT[ok].max():.3e}"
    trunc = truncating_rows(g, key)
    rS = rel_err(np.asarray(u, float), uS)
    okrow = ok if ok.ndim == 1 else ok.all(axis=0)
    if dtype == np.float64:
        # distance to the AS-SHIPPED path (Oracle-S, float32 rounding points included): asserted as a distribution.
        # It cannot be closer than the reference's own fp64 formulas are to its shipped path (uD vs uS), and must
        # not be farther: median and p99 within 10 % of that floor (+ the distance to uD itself), plus absolute caps on the BASELINE configs.
        with np.errstate(invalid="ignore", divide="ignore"):
            floor = rel_err(uD, uS)
        fin = np.isfinite(floor) & np.isfinite(rS)
        for name, f in (("median", np.median), ("p99", lambda x: np.percentile(x, 99))):
            mine, ref = f(rS[fin]), f(floor[fin]) + f(rD[fin])  # row-wise: |u - uS| <= |uD - uS| + |u - uD|
            assert mine <= 1.1 * ref + 1e-9, f"{case_id} [{backend.name}]: {name} vs shipped path {mine:.3e}, reference's own {ref:.3e}"
        cap = SHIPPED_CAPS.get(case_id)
        if cap:
            assert np.median(rS[fin]) <= cap[0] and np.percentile(rS[fin], 99) <= cap[1], \
                f"{case_id} [{backend.name}]: vs shipped path median {np.median(rS[fin]):.3e} p99 {np.percentile(rS[fin], 99):.3e}"
    return dict(case=case_id, worst_vs_D=float(worst), median_vs_D=float(np.median(rD)),
                median_vs_S=float(np.median(rS)), p99_vs_S=float(np.percentile(rS, 99)), n_band=int((~ok).sum()),
                n_trunc=0 if trunc is None else int(trunc[sl].sum()),
                n_trunc_compared=0 if trunc is None else int((trunc[sl] & okrow).sum()))


# ---- AvoidJointLimits / Floating / AvoidObstacles against tests/golden/sec_<arm>.npz
def secondary_limit_params(g, key, n):
    return _abi.make_limits_params(n, g[f"{key}_mn"], g[f"{key}_mx"], g[f"{key}_mt"], g[f"{key}_cz"], g[f"{key}_gr"])


def secondary_obstacle_params(g):
    return _abi.make_obstacles_params(g["obs_obstacles"], float(g["obs_threshold"]), float(g["obs_gain"]))


def check_secondary_against_golden(backend, arm, g, dtype=np.float64):
    """the reference's own outputs (fp64 formulas, `*_uD`); rows at the pinv truncation thresholds
    (floating.py:50-56, avoid_obstacles.py:112) are identified with the oracle's diagnostics."""
    from oracle.oracle import Oracle

    n = backend.n
    o = Oracle(_abi.load_table(arm))
    tol = TOL_D if dtype == np.float64 else TOL_F32
    if arm == "threejoint" and dtype == np.float64:
        tol = TOL_THREEJOINT
    report = {}
    for key in ("limA", "limB"):  # pure function of q: exact up to exp() rounding
        u = np.asarray(backend.limits(secondary_limit_params(g, key, n), g["lim_q"], dtype=dtype), float)
        err = np.max(np.abs(u - g[f"{key}_u"]) / np.maximum(np.abs(g[f"{key}_u"]), 1.0))
        assert err <= (1e-12 if dtype == np.float64 else 1e-3), f"{arm} {key} [{backend.name}]: {err:.3e}"
        report[key] = float(err)
    q, dq = g["float_q"], g["float_dq"]
    for dyn in (0, 1):
        for ts in (0, 1):
            ref = g[f"float_d{dyn}t{ts}_uD"]
            u = np.asarray(backend.floating(dyn, ts, q, dq, dtype=dtype), float)
            _, diag = o.floating_batch(dyn, ts, q, dq)
            ok = (np.abs(np.abs(diag[:, 0]) - 1e-3) > 1e-9) & (np.abs(diag[:, 1] - 1e-4) > 1e-8)
            if dtype != np.float64:
                ok &= diag[:, 1] > 1e-3
            scale = np.maximum(np.max(np.abs(ref), axis=1), 1e-9)  # planar arms: g == 0 exactly
            err = (np.max(np.abs(u - ref), axis=1) / scale)[ok].max()
            assert err <= tol, f"{arm} floating d{dyn} t{ts} [{backend.name}]: {err:.3e}"
            report[f"float_d{dyn}t{ts}"] = float(err)
    P = secondary_obstacle_params(g)
    ref = g["obs_uD"]
    u = np.asarray(backend.obstacles(P, g["obs_q"], dtype=dtype), float)
    _, diag = o.avoid_obstacles_batch(P, g["obs_q"])
    # rows at the pinv truncation threshold, and rows where the reference inverts rounding noise (a closest
    # point on the joint axes it depends on: its output is +-maximum at random, ours is 0)
    ok = (diag[:, 0] > (1e-7 if dtype == np.float64 else 1e-3)) & (diag[:, 1] > (1e-20 if dtype == np.float64 else 1e-8))
    # error relative to the row's signal before np.clip (avoid_obstacles.py:121): clipping at +-maximum
    # would otherwise hide the scale the rounding of the other components lives on
    scale = np.maximum(np.max(np.abs(g["obs_uD_unclipped"]), axis=1), 1e-9)
    err = (np.max(np.abs(u - ref), axis=1) / scale)[ok].max()
    assert err <= tol, f"{arm} obstacles [{backend.name}]: {err:.3e}"
    report["obstacles"] = float(err)
    report["obstacles_band"] = int((~ok).sum())
    return report


def check_oscsec_against_golden(backend, arm, g, dtype=np.float64):
    """OSC with [AvoidJointLimits, AvoidObstacles, Damping] behind its null-space filter (osc.py:310-318):
    the two signals are summed and handed over as u_null_ext, Damping is fused."""
    n = backend.n
    q, dq, t = g["oscsec_q"], g["oscsec_dq"], g["oscsec_target"]
    une = (np.asarray(backend.limits(secondary_limit_params(g, "limA", n), q, dtype=dtype), float)
           + np.asarray(backend.obstacles(secondary_obstacle_params(g), q, dtype=dtype), float))
    params = P(n, kp=100, ctrlr_dof=[int(v) for v in g["oscsec_dof"]], null_controllers=[make_damping(10)])
    u, _ = backend.osc(params, q, dq, t, une=une.astype(dtype), dtype=dtype)
    from oracle.oracle import Oracle

    _, diag = Oracle(_abi.load_table(arm)).avoid_obstacles_batch(secondary_obstacle_params(g), q)
    ok = ~threshold_band(g, "oscsec") & (diag[:, 0] > 1e-7) & (diag[:, 1] > 1e-20)
    tol = TOL_THREEJOINT if arm == "threejoint" else TOL_D
    err = rel_err(np.asarray(u, float), g["oscsec_uD"])[ok].max()
    assert err <= tol, f"{arm} OSC+secondary [{backend.name}]: {err:.3e}"
    return float(err)


DYN_WANTS = ("Tx", "J", "M", "g", "C", "dJ", "R", "T", "quat")
GOLD_KEY = {"Tx": "Tx_EE", "J": "J_EE", "M": "M", "g": "g", "C": "C", "dJ": "dJ_EE", "R": "R_EE", "T": "T_EE",
            "quat": "quat_EE"}


def check_dynamics_against_golden(backend, arm, g, dtype=np.float64):
    """every robot_config function, every frame, zero and non-zero point offsets"""
    n = backend.n
    q, dq = g["dyn_q"], g["dyn_dq"]
    # threejoint: see tolerance note above
    tol = (2e-6 if arm == "threejoint" else 1e-10) if dtype == np.float64 else 2e-4
    scale = lambda ref: max(np.max(np.abs(ref)), 1.0)
    r = backend.dynamics(q, dq, "EE", None, DYN_WANTS, dtype)
    for w in DYN_WANTS:
        ref = g[GOLD_KEY[w]]
        err = np.max(np.abs(np.asarray(r[w], float) - ref)) / scale(ref)
        assert err <= tol, f"{arm} {w}(EE) [{backend.name}]: {err:.3e}"
    if "Tinv_EE" in g:
        r = backend.dynamics(q, dq, "EE", None, ("Tinv",), dtype)
        assert np.max(np.abs(np.asarray(r["Tinv"], float) - g["Tinv_EE"])) <= tol * 10
    want = ("Tx", "J") + (("dJ",) if "dJ_EE_x" in g else ())
    r = backend.dynamics(q, dq, "EE", g["xoff"], want, dtype)
    for w in want:
        ref = g[f"{w}_EE_x"]
        err = np.max(np.abs(np.asarray(r[w], float) - ref)) / scale(ref)
        assert err <= tol, f"{arm} {w}(EE, x) [{backend.name}]: {err:.3e}"
    for f in g["frames"]:
        f = str(f)
        want = ("Tx", "J") + (("R", "dJ") if f"R_{f}" in g else ())
        r = backend.dynamics(q, dq, f, None, want, dtype)
        for w in want:
            ref = g[f"{w}_{f}"]
            err = np.max(np.abs(np.asarray(r[w], float) - ref)) / scale(ref)
            assert err <= tol, f"{arm} {w}({f}) [{backend.name}]: {err:.3e}"


def check_quaternions_all_frames(backend, arm, g, dtype=np.float64):
    """robot_config.R / .quaternion of EVERY frame vs the reference (eigh of the 4x4 K matrix,
    transformations.py:1192-1271); Jaco2's late frames are 6e-4 away from a rotation (tests/golden/quat_<arm>.npz)"""
    worst = 0.0
    for f in g["frames"]:
        f = str(f)
        r = backend.dynamics(g["q"], None, f, None, ("R", "quat"), dtype)
        assert np.max(np.abs(np.asarray(r["R"], float) - g[f"R_{f}"])) <= (1e-12 if dtype == np.float64 else 1e-5)
        qq, ref = np.asarray(r["quat"], float), g[f"quat_{f}"]
        # w >= 0 fixes the sign (transformations.py:1269) except at w == 0, where either sign is the reference's answer
        flip = np.abs(ref[:, 0]) < 1e-9
        err = np.minimum(np.max(np.abs(qq - ref), axis=1), np.where(flip, np.max(np.abs(qq + ref), axis=1), np.inf))
        worst = max(worst, float(err.max()))
    assert worst <= (1e-9 if dtype == np.float64 else 1e-4), f"{arm} quaternion [{backend.name}]: {worst:.3e}"
    return worst


# ---------------------------------------------------------------------------- seeded fuzz over OSC parameters
def fuzz_osc_cases(seed, count, plain_six=False):
    """random (arm table, abrk_osc_params, optional inputs) combinations: joint counts 1..7, orthogonal and
    rounded static transforms, any ctrlr_dof mask, frames, offsets, vmax, ki, target velocity, fused and external
    secondary controllers, both orientation algorithms.
    plain_six: every case is the six-row law with no optional input and no training signal asked for (the `NOTS = true`
    kernels): secondary controllers, integral term, target velocity and external signal are dropped from the draw, and a
    mask that would take the x,y,z / x,y fast path is moved off the end effector frame"""
    from tests.synthetic_arms import make_arm

    rng = np.random.RandomState(seed)
    out = []
    for c in range(count):
        n = int(rng.randint(1, 8))
        tab = make_arm(n, 1000 + seed * 100 + c, non_orthogonal=bool(rng.randint(2)))
        k = int(rng.randint(1, min(n, 6) + 1))
        dof = np.zeros(6, int)
        dof[rng.permutation(6)[:k]] = 1
        frames = ["EE"] + [f"link{i}" for i in range(1, n + 1)] + [f"joint{i}" for i in range(n)]
        nulls = []
        if rng.randint(2):
            nulls.append(make_damping(float(rng.uniform(1, 10))))
        if rng.randint(2):
            rest = [None if rng.randint(2) else float(rng.uniform(0, 6)) for _ in range(n)]
            nulls.append(make_resting(rest, kp=float(rng.uniform(5, 40)), kv=float(rng.uniform(1, 8))))
        kw = dict(kp=float(rng.uniform(5, 200)), ko=float(rng.uniform(5, 150)), kv=float(rng.uniform(2, 25)),
                  ki=float(rng.uniform(0.05, 0.5)) if rng.randint(3) == 0 else 0,
                  vmax=[float(rng.uniform(0.2, 2)), float(rng.uniform(0.2, 2))] if rng.randint(3) == 0 else None,
                  ctrlr_dof=dof.tolist(), null_controllers=nulls, use_g=bool(rng.randint(2)), use_C=bool(rng.randint(2)),
                  orientation_algorithm=int(rng.randint(2)), ref_frame=frames[rng.randint(len(frames))],
                  xyz_offset=rng.uniform(-0.2, 0.2, 3).tolist() if rng.randint(2) else None)
        tv, ext, row_seed = bool(rng.randint(3) == 0), bool(rng.randint(3) == 0), int(rng.randint(1 << 30))
        if plain_six:
            tv = ext = False
            kw.update(null_controllers=[], ki=0)
            d = kw["ctrlr_dof"]
            if kw["ref_frame"] == "EE" and (d == XYZ or (d == XY and n <= 3)):
                kw["ref_frame"] = f"link{n}"
            out.append(dict(tab=tab, n=n, kw=kw, tv=False, ext=False, seed=row_seed, ts=False))
            continue
        # whether the call asks for the training signal (osc.py:297): drawn per case from the row seed's parity, so that
        # the cases of earlier rounds keep their arms / parameters / rows.  Without it the plain six-row law runs its NoTs
        # instantiations - what bench.py and a C-ABI caller without that buffer get
        out.append(dict(tab=tab, n=n, kw=kw, tv=tv, ext=ext, seed=row_seed, ts=bool(row_seed & 1)))
    return out


def check_fuzz_case(backend_factory, fc, B=96):
    """one fuzz case on a backend vs the oracle; rows near the `_Mx` thresholds or with an ill-conditioned M /
    Mx_inv (where 1e-6 is not attainable in fp64 by either side) are left out"""
    from oracle.oracle import Oracle

    n, tab = fc["n"], fc["tab"]
    rng = np.random.RandomState(fc["seed"])
    q, dq, t = rng.uniform(-3, 3, (B, n)), rng.uniform(-2, 2, (B, n)), rng.uniform(-0.6, 0.6, (B, 6))
    tv = rng.uniform(-0.5, 0.5, (B, 6)) if fc["tv"] else None
    une = rng.uniform(-2, 2, (B, n)) if fc["ext"] else None
    params = P(n, **fc["kw"])
    o = Oracle(tab)
    ie_o = np.zeros((B, 6)) if params.ki != 0 else None
    uo = o.osc_batch(params, q, dq, t, tv, ie_o, une)
    be = backend_factory(tab)
    if hasattr(be, "training_signal"):
        be.training_signal = fc.get("ts", True)
    ie = np.zeros((B, 6)) if params.ki != 0 else None
    u, _ = be.osc(params, q, dq, t, tv, ie=ie, une=une)
    dof = np.array(fc["kw"]["ctrlr_dof"], bool)
    ok = np.ones(B, bool)
    for b in range(B):
        M = o.M(q[b])
        J = o.J(fc["kw"]["ref_frame"], q[b], fc["kw"]["xyz_offset"])[dof]
        if np.linalg.cond(M) > 1e7:
            ok[b] = False
            continue
        A = J @ np.linalg.inv(M) @ J.T
        sv = np.linalg.svd(A, compute_uv=False)
        det = abs(np.linalg.det(A))
        # (a frame no joint moves - joint0, link0 - has J = 0: an all-zero Mx_inv sits at neither threshold)
        near = abs(det - 1e-3) < 1e-8 or (det < 1.001e-3 and sv.max() > 0 and np.any(np.abs(sv / sv.max() - 1e-4) < 1e-8))
        # below the det threshold the law uses a truncated pinv: well-posed only if the kept part is well separated
        if near or (sv.max() / max(sv.min(), 1e-300) > 1e7 and det >= 1e-3):
            ok[b] = False
    u = np.asarray(u, float)
    # a frame no joint moves (joint0, link0) has J = 0: the law returns 0 on both sides - exactly, or as rounding
    # noise of analytically vanishing terms (C dq of a one-joint arm, ~1e-16).  Those rows are compared absolutely
    # (the relative metric would be 0/0 or noise/noise)
    zero = np.max(np.abs(uo), axis=1) < 1e-12
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(zero, np.max(np.abs(u - uo), axis=1), rel_err(u, uo))
    assert ok.sum() >= B // 2, f"fuzz case filtered too hard ({ok.sum()}/{B})"
    assert err[ok].max() <= TOL_D, f"fuzz n={n} {fc['kw']}: {err[ok].max():.3e} (row {int(np.argmax(np.where(ok, err, 0)))})"
    if ie is not None:
        assert np.allclose(ie[ok], ie_o[ok], rtol=1e-9, atol=1e-12)
    return float(err[ok].max())


def check_six_row_use_C(backend, arm="ur5", B=400):
    """orientation control + Coriolis compensation on a built-in (orthogonal-chain) arm vs the oracle: the six-row
    kernels compute C(q,dq) dq in a pass of their own"""
    from oracle.oracle import Oracle

    o = Oracle(_abi.load_table(arm))
    n = o.n
    rng = np.random.RandomState(17)
    q, dq, t = rng.uniform(0, 6.28, (B, n)), rng.uniform(-2, 2, (B, n)), rng.uniform(-0.8, 0.8, (B, 6))
    worst = 0.0
    for kw in (dict(kp=100, ko=60, kv=12, ctrlr_dof=SIX, use_C=True),
               dict(kp=100, ko=60, kv=12, ctrlr_dof=[1, 0, 1, 0, 1, 0] if n > 3 else [1, 1, 0, 0, 0, 1], use_C=True,
                    orientation_algorithm=1,
                    ref_frame=f"link{n - 1}" if n > 3 else "EE", xyz_offset=[0.05, 0.0, -0.1] if n > 3 else [0.05, 0.1, 0],
                    null_controllers=[make_damping(5)]),
               dict(kp=50, ki=0.1, ctrlr_dof=XYZ if n > 3 else XY, use_C=True, vmax=[0.6, 1.0])):
        if n < 6 and sum(kw["ctrlr_dof"]) > n:
            continue
        p = P(n, **kw)
        ie_o = np.zeros((B, 6)) if kw.get("ki") else None
        ie = np.zeros((B, 6)) if kw.get("ki") else None
        uo = o.osc_batch(p, q, dq, t, None, ie_o, None)
        u, _ = backend.osc(p, q, dq, t, ie=ie)
        ok = np.ones(B, bool)
        dof = np.array(kw["ctrlr_dof"], bool)
        for b in range(B):
            J = o.J(kw.get("ref_frame", "EE"), q[b], kw.get("xyz_offset"))[dof]
            A = J @ np.linalg.inv(o.M(q[b])) @ J.T
            sv = np.linalg.svd(A, compute_uv=False)
            det = abs(np.linalg.det(A))
            ok[b] = not (abs(det - 1e-3) < 1e-8 or (det < 1.001e-3 and np.any(np.abs(sv / sv.max() - 1e-4) < 1e-8))
                         or sv.max() / max(sv.min(), 1e-300) > 1e9)
        err = rel_err(np.asarray(u, float), uo)[ok].max()
        assert err <= TOL_D, f"{arm} six-row use_C {kw}: {err:.3e}"
        worst = max(worst, err)
    return worst


_NEAR_SINGULAR = {}


def near_singular_postures(arm="ur5", B=600):
    """B joint states of `arm` whose x,y,z task-space inertia is nearly singular, the ratio of its extreme singular
    values spread evenly (in the exponent) over 1e-13 .. 3e-3: the iterates of a seeded Nelder-Mead descent on that ratio
    from random postures (the oracle evaluates it).  Deterministic; cached per process."""
    if (arm, B) in _NEAR_SINGULAR:
        return _NEAR_SINGULAR[(arm, B)]
    from scipy.optimize import minimize

    from oracle.oracle import Oracle

    o = Oracle(_abi.load_table(arm))
    n = o.n

    def ratio(q):
        J = o.J("EE", q, None)[:3]
        sv = np.linalg.svd(J @ np.linalg.inv(o.M(q)) @ J.T, compute_uv=False)
        return sv.min() / sv.max()

    rng = np.random.RandomState(23)
    seen = []

    def f(q):
        r = ratio(q)
        seen.append((r, q.copy()))
        return np.log(r + 1e-300)

    for _ in range(40):
        minimize(f, rng.uniform(0, 6.28, n), method="Nelder-Mead", options=dict(maxiter=600, xatol=1e-12, fatol=1e-12))
    r = np.array([x[0] for x in seen])
    qs = np.array([x[1] for x in seen])
    keep = (r < 3e-3) & (r > 1e-13)
    r, qs = r[keep], qs[keep]
    bins = np.clip(((np.log10(r) + 13) / (13 + np.log10(3e-3)) * 30).astype(int), 0, 29)
    pick = []
    for b in range(30):
        idx = np.flatnonzero(bins == b)
        pick += list(rng.choice(idx, min(len(idx), B // 30), replace=False))
    q = qs[np.array(pick)]
    _NEAR_SINGULAR[(arm, B)] = q
    return q


def check_near_singular_postures(backend, arm="ur5", B=600):
    """the x,y,z law on postures that approach the arm's kinematic singularities (near_singular_postures): Mx_inv
    there has one or two eigenvalues far below the others, i.e. exactly where the cofactor form of Mx loses accuracy
    and osc_law falls back to its Cholesky factor (trace^3 / det > 1e6) - and where the truncating pinv takes over.
    Against the oracle; rows within 1e-8 of a threshold of `_Mx` are excluded, and so are rows whose kept part of
    Mx_inv is itself ill-conditioned beyond 1e7 (neither side is good to 1e-6 there).
    -> (worst relative error, number of rows beyond the accuracy gate, number of truncating rows)"""
    from oracle.oracle import Oracle

    o = Oracle(_abi.load_table(arm))
    n = o.n
    q = near_singular_postures(arm, B)
    B = q.shape[0]
    rng = np.random.RandomState(29)
    dq, t = rng.uniform(-2, 2, (B, n)), rng.uniform(-0.8, 0.8, (B, 6))
    worst, beyond, trunc = 0.0, 0, 0
    for kw in (dict(kp=200), dict(kp=120, kv=15, use_C=True, null_controllers=[make_damping(8)])):
        p = P(n, **kw)
        uo = o.osc_batch(p, q, dq, t, None, None, None)
        u, _ = backend.osc(p, q, dq, t)
        ok = np.ones(B, bool)
        for b in range(B):
            J = o.J("EE", q[b], None)[:3]
            A = J @ np.linalg.inv(o.M(q[b])) @ J.T
            sv = np.linalg.svd(A, compute_uv=False)
            det = abs(np.linalg.det(A))
            ratio = sv / sv.max()
            near = abs(det - 1e-3) < 1e-8 or (det < 1.001e-3 and np.any(np.abs(ratio - 1e-4) < 1e-8))
            kept = ratio[ratio > 1e-4] if det < 1e-3 else ratio
            ok[b] = not near and kept.min() > 1e-7
            beyond += int(np.trace(A) ** 3 > 1e6 * det)
            trunc += int(det < 1e-3 and ratio.min() < 1e-4)
        assert ok.sum() > B // 2, f"near-singular set filtered too hard ({ok.sum()}/{B})"
        err = rel_err(np.asarray(u, float), uo)[ok].max()
        assert err <= TOL_D, f"{arm} near-singular {kw}: {err:.3e}"
        worst = max(worst, err)
    return worst, beyond, trunc


def six_row_gate(o, q, ctrlr_dof=SIX, frame="EE", offset=None):
    """per row of `q`, from the task-space inertia inverse Mx_inv = J M^-1 J^T of the controlled rows (`o` an Oracle):
    ok - the row is good to TOL_D on both sides in fp64: not within 1e-8 of a threshold of `_Mx` (osc.py:138-145), and the
    part of Mx_inv the pinv keeps is conditioned below 1e7; trunc - `pinv(Mx_inv, rcond=1e-4)` really drops a singular
    value (|det| < 1e-3 and min(sv) < 1e-4 max(sv)): the rows the six-row kernels defer to their second pass; cond - the
    condition number of Mx_inv.  -> (ok, trunc, cond), arrays over the rows"""
    dof = np.array(ctrlr_dof, bool)
    B = len(q)
    ok, trunc, cond = np.ones(B, bool), np.zeros(B, bool), np.zeros(B)
    for b in range(B):
        J = o.J(frame, q[b], offset)[dof]
        A = J @ np.linalg.inv(o.M(q[b])) @ J.T
        sv = np.linalg.svd(A, compute_uv=False)
        det = abs(np.linalg.det(A))
        ratio = sv / sv.max()
        near = abs(det - 1e-3) < 1e-8 or (det < 1.001e-3 and np.any(np.abs(ratio - 1e-4) < 1e-8))
        kept = ratio[ratio > 1e-4] if det < 1e-3 else ratio
        ok[b] = not near and kept.min() > 1e-7
        trunc[b] = det < 1e-3 and ratio.min() < 1e-4
        cond[b] = sv.max() / max(sv.min(), 1e-300)
    return ok, trunc, cond


def check_six_row_near_singular(backend, arm="ur5", B=600, reference=None):
    """all six task rows on postures next to the arm's kinematic singularities (near_singular_postures): most of them
    take the truncating pinv(rcond=1e-4) of osc.py:145, i.e. the path the six-row kernels defer to their second pass.
    Plain law, Coriolis term + fused secondary controllers, and every optional input (target velocity, integral
    state over two steps, external null-space signal) against the oracle; `reference` (a second backend, e.g. the
    inline form of the same row programs) must agree to 1e-9 where given.
    -> (worst relative error vs the oracle, truncating rows compared)"""
    from oracle.oracle import Oracle

    o = Oracle(_abi.load_table(arm))
    n = o.n
    q = near_singular_postures(arm, B)
    B = q.shape[0]
    rng = np.random.RandomState(31)
    dq, t = rng.uniform(-2, 2, (B, n)), rng.uniform(-0.8, 0.8, (B, 6))
    tv, une = rng.uniform(-0.5, 0.5, (B, 6)), rng.uniform(-2, 2, (B, n))
    ok, trunc, _cond = six_row_gate(o, q)
    assert (ok & trunc).sum() > B // 4, f"too few truncating rows ({(ok & trunc).sum()}/{B})"
    worst = 0.0
    variants = (dict(kw=dict(kp=200, ko=150, kv=25, ctrlr_dof=SIX)),
                dict(kw=dict(kp=120, ko=90, kv=15, ctrlr_dof=SIX, use_C=True, orientation_algorithm=1,
                             null_controllers=[make_damping(8), make_resting([None, 0.8, -1.6, None, 1.5, None][:n] +
                                                                                [None] * max(0, n - 6), kp=40, kv=8)])),
                dict(kw=dict(kp=100, ko=60, kv=12, ki=0.2, ctrlr_dof=SIX, vmax=[0.5, 1.0], use_g=False), tv=True, ext=True,
                     steps=2))
    for v in variants:
        p = P(n, **v["kw"])
        steps = v.get("steps", 1)
        ie_o = np.zeros((B, 6)) if p.ki != 0 else None
        ie = np.zeros((B, 6)) if p.ki != 0 else None
        ie_r = np.zeros((B, 6)) if p.ki != 0 else None
        for _ in range(steps):
            uo = o.osc_batch(p, q, dq, t, tv if v.get("tv") else None, ie_o, une if v.get("ext") else None)
            u, _ts = backend.osc(p, q, dq, t, tv if v.get("tv") else None, ie=ie, une=une if v.get("ext") else None)
            err = rel_err(np.asarray(u, float), uo)[ok].max()
            assert err <= TOL_D, f"{arm} six rows near-singular {v['kw']} [{backend.name}]: {err:.3e}"
            worst = max(worst, err)
            if reference is not None:
                ur, _ = reference.osc(p, q, dq, t, tv if v.get("tv") else None, ie=ie_r, une=une if v.get("ext") else None)
                d = rel_err(np.asarray(u, float), np.asarray(ur, float))[ok].max()
                assert d <= 1e-9, f"{arm} six rows near-singular {v['kw']}: {backend.name} vs {reference.name} {d:.3e}"
        if ie is not None:
            assert np.allclose(ie, ie_o, rtol=1e-9, atol=1e-12)
    return worst, int((ok & trunc).sum())


# ---------------------------------------------------------------------------- seeded fuzz: Sliding / Joint / dynamics
def check_fuzz_other(backend_factory, seed, B=64):
    """Sliding (Cartesian with frames/offsets/velocity+acceleration targets, joint space), Joint, Damping,
    RestingConfig and every robot_config output on one random user arm vs the oracle"""
    from oracle.oracle import Oracle
    from tests.synthetic_arms import make_arm

    rng = np.random.RandomState(seed)
    n = int(rng.randint(1, 8))
    tab = make_arm(n, 5000 + seed, non_orthogonal=bool(rng.randint(2)))
    o, be = Oracle(tab), backend_factory(tab)
    q, dq = rng.uniform(-3, 3, (B, n)), rng.uniform(-2, 2, (B, n))
    frames = ["EE"] + [f"link{i}" for i in range(1, n + 1)] + [f"joint{i}" for i in range(n)]
    worst = {}
    # Sliding: the reference's pinv(J[:3]) has rcond 1e-15 - rows whose J[:3] is ill-conditioned amplify rounding on
    # both sides and are left out
    frame = frames[rng.randint(len(frames))]
    off = rng.uniform(-0.2, 0.2, 3).tolist() if rng.randint(2) else None
    sp = SP(n, kd=float(rng.uniform(5, 200)), lamb=float(rng.uniform(1, 40)), cartesian=True, ref_frame=frame, offset=off)
    t3 = rng.uniform(-0.6, 0.6, (B, 3))
    tv, ta = (rng.uniform(-1, 1, (B, 3)), rng.uniform(-1, 1, (B, 3))) if rng.randint(2) else (None, None)
    uo, so = o.sliding_batch(sp, q, dq, t3, tv, ta)
    u, s = backend_factory(tab).sliding(sp, q, dq, t3, tv, ta)
    sv = np.array([np.linalg.svd(o.J(frame, q[b], off)[:3], compute_uv=False) for b in range(B)])
    rank = (sv > 1e-9 * sv.max(axis=1, keepdims=True)).sum(axis=1)
    full = rank == rank.max()
    smin = np.array([sv[b][rank[b] - 1] for b in range(B)])
    ok = full & (sv.max(axis=1) / smin < 1e4)
    if ok.sum() >= 8:
        worst["sliding"] = float(rel_err(np.asarray(u, float), uo)[ok].max())
        assert worst["sliding"] <= TOL_D and rel_err(np.asarray(s, float), so)[ok].max() <= TOL_D, (seed, n, worst)
    spj = SP(n, kd=12.0, lamb=3.0, cartesian=False)
    tn, tvn, tan = rng.uniform(-2, 2, (B, n)), rng.uniform(-1, 1, (B, n)), rng.uniform(-1, 1, (B, n))
    uo, _ = o.sliding_batch(spj, q, dq, tn, tvn, tan)
    u, _ = be.sliding(spj, q, dq, tn, tvn, tan)
    worst["sliding_joint"] = float(rel_err(np.asarray(u, float), uo).max())
    assert worst["sliding_joint"] <= TOL_D, (seed, n, worst)
    for name, ctrl, grav, tt, tvv in (("joint", make_joint(30, 6), True, tn, tvn), ("damping", make_damping(7), False, None, None),
                                      ("resting", make_resting([None if i % 2 else 0.5 * i for i in range(n)], kp=20, kv=4),
                                       False, None, None)):
        uo = o.joint_batch(ctrl, grav, q, dq, tt, tvv)
        u = be.joint(ctrl, grav, q, dq, tt, tvv)
        worst[name] = float(np.max(np.abs(np.asarray(u, float) - uo)) / max(np.max(np.abs(uo)), 1e-9))
        assert worst[name] <= 1e-10, (seed, n, worst)
    f2 = frames[rng.randint(len(frames))]
    want = ("Tx", "J", "dJ", "M", "g", "C", "R", "T", "Tinv", "quat")
    r = be.dynamics(q, dq, f2, off, want)
    ro = OracleBackend.__new__(OracleBackend)
    ro.o, ro.n = o, n
    ref = ro.dynamics(q, dq, f2, off, tuple(w for w in want if w not in ("T", "Tinv")))
    for w, v in ref.items():
        err = np.max(np.abs(np.asarray(r[w], float) - v)) / max(np.max(np.abs(v)), 1.0)
        assert err <= 1e-10, (seed, n, f2, w, err)
    return worst


def check_fuzz_secondary(backend_factory, seed, B=64):
    """AvoidJointLimits (random limits, gradient / cross_zero flags, missing limits), Floating (all four modes) and
    AvoidObstacles (random obstacles, threshold, gain) on one random user arm vs the oracle"""
    from oracle.oracle import Oracle, avoid_joint_limits_batch
    from tests.synthetic_arms import make_arm

    rng = np.random.RandomState(seed)
    n = int(rng.randint(1, 8))
    tab = make_arm(n, 9000 + seed, non_orthogonal=bool(rng.randint(2)))
    o, be = Oracle(tab), backend_factory(tab)
    q, dq = rng.uniform(-3.5, 3.5, (B, n)), rng.uniform(-2, 2, (B, n))
    worst = {}
    # ---- AvoidJointLimits
    lo = rng.uniform(0.2, 3.0, n)
    hi = lo + rng.uniform(0.3, 3.0, n)
    mn = [None if rng.rand() < 0.2 else float(v) for v in lo]
    mx = [None if rng.rand() < 0.2 else float(v) for v in hi]
    PL = _abi.make_limits_params(n, mn, mx, list(rng.uniform(0.5, 50, n)), list(rng.rand(n) < 0.3),
                                 list(rng.rand(n) < 0.4))
    with np.errstate(all="ignore"):
        want = avoid_joint_limits_batch(n, PL, q)
    got = np.asarray(be.limits(PL, q), float)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12), f"limits seed {seed} n={n}"
    # ---- Floating
    for dyn in (0, 1):
        for ts in (0, 1):
            uo, diag = o.floating_batch(dyn, ts, q, dq)
            ok = (np.abs(np.abs(diag[:, 0]) - 1e-3) > 1e-9) & (np.abs(diag[:, 1] - 1e-4) > 1e-8)
            for b in range(B):  # ill-conditioned M / task inertia: 1e-9 is not attainable by either side
                M = o.M(q[b])
                if np.linalg.cond(M) > 1e6:
                    ok[b] = False
            u = np.asarray(be.floating(dyn, ts, q, dq), float)
            zero = np.max(np.abs(uo), axis=1) < 1e-12
            with np.errstate(invalid="ignore", divide="ignore"):
                err = np.where(zero, np.max(np.abs(u - uo), axis=1), rel_err(u, uo))
            if ok.any():
                worst[f"floating{dyn}{ts}"] = float(err[ok].max())
                assert err[ok].max() < 1e-6, f"floating seed {seed} n={n} dyn={dyn} ts={ts}: {err[ok].max():.3e}"
    # ---- AvoidObstacles
    k = int(rng.randint(1, 5))
    obstacles = np.column_stack([rng.uniform(-0.8, 0.8, (k, 3)), rng.uniform(0.02, 0.2, k)])
    PO = _abi.make_obstacles_params(obstacles=obstacles, threshold=float(rng.uniform(0.1, 0.6)),
                                    gain=float(rng.uniform(1, 50)))
    with np.errstate(all="ignore"):
        uo, diag = o.avoid_obstacles_batch(PO, q)
    # mobility (diag[:, 1]): a closest point that barely moves with the joints it hangs on has a task-space inertia
    # made of rounding noise, which both sides invert differently (the golden check keeps its documented 1e-20 floor;
    # random arms reach 1e-14, e.g. seed 15600)
    ok = (diag[:, 0] > 1e-7) & (diag[:, 1] > 1e-12)
    for b in range(B):
        if np.linalg.cond(o.M(q[b])) > 1e6:
            ok[b] = False
    u = np.asarray(be.obstacles(PO, q), float)
    if ok.any():
        scale = np.maximum(np.max(np.abs(uo), axis=1), 1e-6)
        err = np.max(np.abs(u - uo), axis=1) / scale
        worst["obstacles"] = float(err[ok].max())
        assert err[ok].max() < 1e-5, f"obstacles seed {seed} n={n} k={k}: {err[ok].max():.3e} (row {int(np.argmax(np.where(ok, err, 0)))})"
    return worst
