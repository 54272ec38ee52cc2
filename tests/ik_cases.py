"""Inputs, reference and bars of the inverse-kinematics tests (tests/test_ik_hostsim.py on the CPU, tests/test_ik_gpu.py
on the device).  The reference is the C oracle (oracle.ik_paths, Oracle.J / Tx / quaternion); neither the kernels nor
their host build enter any bar.

One step of InverseKinematics.generate_path is  dq = f(J, dx, dr)  with f one of three formulas that invert J, J J^T +
0.001 I, or the blocks J[:3] and J[3:].  A step computed in dtype T therefore carries an error of about
eps_T * kappa * scale, kappa the condition number of what is inverted (over the singular values numpy.linalg.pinv keeps
at rcond = 1e-15) and scale the size of the terms that are added up.  `one_step` returns the oracle's step together with
kappa, scale and the flags that say whether a (row, step) pair can be held to the bar at all.  The bar is
C * eps_T * (kappa * scale + extra): `extra` is the residual term of the least-squares perturbation bound and the
rounding of dx = target - Tx(q) and dr, which kappa * scale leaves out (derivation and what plain NumPy needs with and
without it: profiles/ik_tests.md).

  not counted: kappa above KAPPA_GATE[T]; a singular value within a factor 10 of the rcond cut (either implementation
  may keep or drop it); |Qe[0]| below W_GATE[T] (quaternion_from_matrix returns w >= 0, so the sign of the whole
  quaternion, and with it of dr, is decided by rounding there); a clamp comparison within CLAMP_BAND[T] of its limit.

The share of pairs left out of a random-posture case is capped (CAP) and asserted on the reference before anything is
compared.  `numpy_step` evaluates the same three formulas in plain NumPy in dtype T from the oracle's J, dx and dr rounded
to T: what it needs of C on the counted pairs is recorded in profiles/ik_tests.md and C is at least four times that
(tests/test_ik_hostsim.py asserts it).

`teacher_forced` holds every stored step of a path to the bar from the path's own position, so nothing grows along it."""
import ctypes as C_
import functools
import types

import numpy as np

from abr_control_amd import _abi
from oracle import oracle as O

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
C = 64.0  # the bar's constant; numpy_step needs at most C / 4 of it on the counted pairs (profiles/ik_tests.md)
KAPPA_GATE = {F32: 1e3, F64: 1e7}
# Method 2 inverts J J^T + 0.001 I, whose condition number (smax^2 + 0.001) / (smin^2 + 0.001) is at least 1001 on every
# arm of fewer than six joints (J J^T is singular) and above 1e3 on about half the postures of the others: under 1e3 the
# float32 comparison would be empty.  The damping also bounds it, by 1 + 1000 smax^2, at every posture; so float32 counts
# method 2 up to the kappa at which the bar is a quarter of the scale, C eps32 kappa = 0.25: beyond it a comparison
# says little, below it a wrong factor or sign in the formula still fails.
KAPPA_GATE_DAMPED_F32 = 0.25 / (64.0 * 2.0 ** -23)  # 3.3e4
W_GATE = {F32: 1e-3, F64: 1e-9}
CLAMP_BAND = {F32: 1e-5, F64: 1e-12}
FAST_GATE = {F32: 1e2, F64: 1e6}  # pinv_KxN takes its Cholesky path where trace^K < det * this
CAP = 0.05
RCOND = 1e-15
# "slow" is there for the max_dq clamp alone: a one-joint arm cannot reach it under the other two (|dq| <= max_dx dt / |Jx|)
LIMITS = {"default": {}, "wide": dict(max_dx=50.0, max_dr=300.0, max_dq=2000.0), "slow": dict(max_dq=0.05)}
N_SINGULAR, N_NEAR = 16, 8
# chosen so that the oracle alone meets CAP in every case of both test files (a case asserts it before it runs anything)
SEED_STEP, SEED_PATH = 1, 3


def eps(dtype):
    return float(np.finfo(np.dtype(dtype)).eps)


def params(limits, method, T=1, dt=0.001, **over):
    kw = dict(LIMITS[limits] if isinstance(limits, str) else limits)
    kw.update(over)
    return _abi.make_ik_params(n_timesteps=T, dt=dt, method=method, **kw)


def table(arm):
    """a built-in arm's name or a table dict -> the table"""
    return _abi.load_table(arm) if isinstance(arm, str) else arm


@functools.lru_cache(maxsize=None)
def synthetic(n):
    from tests.synthetic_arms import make_arm

    return make_arm(n, 70 + n)


def _round(a, dtype):
    return np.ascontiguousarray(np.asarray(a, dtype=np.dtype(dtype)).astype(np.float64))


def _tx(o, q):
    return np.array([o.Tx("EE", qb) for qb in q])


def euler_sxyz(R):
    """the static-frame x, y, z angles of a rotation matrix (R = Rz(c) Ry(b) Rx(a)), away from b = +-pi / 2"""
    return np.array([np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], np.hypot(R[0, 0], R[1, 0])),
                     np.arctan2(R[1, 0], R[0, 0])])


def draw_random(arm, B, seed, dtype):
    """q ~ U(-3, 3), target xyz ~ U(-0.5, 0.5), Euler ~ U(-3, 3), rounded to dtype -> (q, target, block); block[b] is
    0 for the singular block (the first 16 rows: every angle a multiple of pi / 2, in one wavefront with 48 random rows),
    2 for the last 8 rows, whose target is the pose 0.5 .. 3 cm and 0.05 .. 0.3 rad from where the arm is (at random
    targets the wide max_dx and max_dr clamp on nearly every row of a one-step case; these rows are the other side),
    1 for the others.  Batches shorter than 32 rows hold random rows only."""
    tab = table(arm)
    n = tab["n_joints"]
    r = np.random.RandomState(seed)
    q, xyz, abg = r.uniform(-3, 3, (B, n)), r.uniform(-0.5, 0.5, (B, 3)), r.uniform(-3, 3, (B, 3))
    k, d, ln = r.randint(-2, 3, (N_SINGULAR, n)), r.normal(size=(N_NEAR, 2, 3)), r.uniform(0, 1, (N_NEAR, 2))
    block = np.ones(B, dtype=int)
    if B >= 2 * N_SINGULAR:
        q[:N_SINGULAR] = k * (np.pi / 2)
        block[:N_SINGULAR], block[-N_NEAR:] = 0, 2
    q = _round(q, dtype)
    if B >= 2 * N_SINGULAR:
        o = O.Oracle(tab)
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        for i, b in enumerate(range(B - N_NEAR, B)):
            xyz[b] = o.Tx("EE", q[b]) + d[i, 0] * (0.005 + 0.025 * ln[i, 0])
            v = d[i, 1] * (0.05 + 0.25 * ln[i, 1])  # rotation vector -> matrix (Rodrigues)
            th, K = np.linalg.norm(v), np.cross(np.eye(3), v / np.linalg.norm(v))
            abg[b] = euler_sxyz((np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K) @ o.R("EE", q[b]))
    return q, _round(np.hstack([xyz, abg]), dtype), block


def draw_reachable(arm, B, seed, dtype):
    """q0 ~ U(0.3, 2.8), target xyz = Tx(EE, q0 + U(-0.3, 0.3)), Euler ~ U(-3, 3), rounded to dtype -> (q0, target)"""
    tab = table(arm)
    n = tab["n_joints"]
    r = np.random.RandomState(seed)
    q0 = r.uniform(0.3, 2.8, (B, n))
    xyz = _tx(O.Oracle(tab), q0 + r.uniform(-0.3, 0.3, (B, n)))
    return _round(q0, dtype), _round(np.hstack([xyz, r.uniform(-3, 3, (B, 3))]), dtype)


def _quat_sxyz(abg):
    out = np.zeros((len(abg), 4))
    f = O.lib().abrk_oracle_quat_from_euler_sxyz
    for b, (x, y, z) in enumerate(abg):
        f(C_.c_double(x), C_.c_double(y), C_.c_double(z), out[b].ctypes.data_as(C_.POINTER(C_.c_double)))
    return out / np.linalg.norm(out, axis=1, keepdims=True)


def blocks(J, method):
    """what the method inverts: J [B,6,n] -> list of [B,k,m] arrays"""
    if method == 1:
        return [J]
    if method == 2:
        return [J @ J.transpose(0, 2, 1) + 0.001 * np.eye(6, dtype=J.dtype)]
    return [J[:, :3], J[:, 3:]]


def numpy_step(J, dx, dr, method, max_dq, dtype):
    """inverse_kinematics.py:104-130 in plain NumPy on arrays of `dtype`: J [B,6,n], dx, dr [B,3] (already clamped)
    -> (dq after the max_dq clamp, largest |dq_i| before it, the terms that are summed [B,k,n])"""
    dt = np.dtype(dtype)
    J, dx, dr = (np.asarray(a, dtype=np.float64).astype(dt) for a in (J, dx, dr))
    n = J.shape[2]
    mv = lambda A, v: (A @ v[:, :, None])[:, :, 0]
    if method == 1:
        dq = mv(np.linalg.pinv(J, rcond=RCOND), np.concatenate([dx, dr], axis=1))
        terms = dq[:, None]
    elif method == 2:
        A = J @ J.transpose(0, 2, 1) + dt.type(0.001) * np.eye(6, dtype=dt)
        rhs = np.concatenate([dx, dr * dt.type(0.3)], axis=1)
        dq = mv(J.transpose(0, 2, 1), np.linalg.solve(A, rhs[:, :, None])[:, :, 0])
        terms = dq[:, None]
    else:
        Jx, Jw = J[:, :3], J[:, 3:]
        pJx, pJw = np.linalg.pinv(Jx, rcond=RCOND), np.linalg.pinv(Jw, rcond=RCOND)
        a, b = mv(pJx, dx), mv(pJw, dr)
        dq = a + mv(np.eye(n, dtype=dt) - pJx @ Jx, b)
        terms = np.stack([a, b, dq], axis=1)
    assert dq.dtype == dt
    m = np.abs(dq).max(axis=1)
    lim = dt.type(max_dq)
    sc = np.where(m > lim, lim / np.where(m > 0, m, 1), dt.type(1)).astype(dt)
    return dq * sc[:, None], m, terms


def one_step(tab, p, q, tgt):
    """One oracle step from every row of q [B,n] towards tgt [B,6] with the limits and method of `p` -> namespace of
    per-row arrays: dq_ref [B,n]; sv: list of the singular values of each inverted block; kappa; scale; near_cut;
    clamp_dx / clamp_dr / clamp_dq (engaged?) and near_limit (a clamp comparison within 1e-12 .. 1e-5 of its limit, as
    the relative distance); gate [B, blocks]: trace^K / det of each block's Gram matrix where pinv_KxN has a fast path
    (inf where it has none); w = |Qe[0]|; J, dx, dr (clamped) for numpy_step"""
    tab = table(tab)
    q, tgt = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(tgt, dtype=np.float64)
    o = O.Oracle(tab)
    B, n, method = len(q), o.n, int(p.method)
    p1 = _abi.make_ik_params(p.max_dx, p.max_dr, p.max_dq, 1, p.dt, method)
    dq_ref = O.ik_paths(tab, p1, q, tgt)[1][:, 0]
    J = np.array([o.J("EE", qb) for qb in q]).reshape(B, 6, n)
    Qe = np.array([o.quaternion("EE", qb) for qb in q]).reshape(B, 4)
    Qd = _quat_sxyz(tgt[:, 3:])
    dx = tgt[:, :3] - _tx(o, q).reshape(B, 3)
    dx0 = dx.copy()
    dr = Qe[:, :1] * Qd[:, 1:] - Qd[:, :1] * Qe[:, 1:] - np.cross(Qd[:, 1:], Qe[:, 1:])
    lim = dict(dx=p.max_dx * p.dt, dr=p.max_dr * p.dt, dq=p.max_dq * p.dt)
    size = dict(dx=np.linalg.norm(dx, axis=1), dr=np.linalg.norm(dr, axis=1))
    for k, v in (("dx", dx), ("dr", dr)):
        on = size[k] > lim[k]
        v[on] *= (lim[k] / size[k][on])[:, None]
    dq64, size["dq"], terms = numpy_step(J, dx, dr, method, lim["dq"], F64)
    r = types.SimpleNamespace(dq_ref=dq_ref, J=J, dx=dx, dr=dr, w=np.abs(Qe[:, 0]), method=method, lim=lim, dq64=dq64)
    for k in lim:
        setattr(r, "clamp_" + k, size[k] > lim[k])
    r.near_limit = np.min([np.abs(size[k] / lim[k] - 1) for k in lim], axis=0)
    r.sv = [np.linalg.svd(b, compute_uv=False) for b in blocks(J, method)]
    r.kappa, r.near_cut, gate, smin = np.zeros(B), np.zeros(B, dtype=bool), [], []
    for s, blk in zip(r.sv, blocks(J, method)):
        smax = s.max(axis=1, keepdims=True)
        kept = s > RCOND * smax
        smin.append(np.where(kept, s, np.inf).min(axis=1))
        r.kappa += np.where(smax[:, 0] > 0, smax[:, 0] / smin[-1], 1.0)
        r.near_cut |= ((s > 0.1 * RCOND * smax) & (s < 10 * RCOND * smax)).any(axis=1)
        K = blk.shape[1]
        if method == 2 or K > n:
            gate.append(np.full(B, np.inf))
        else:
            G = blk @ blk.transpose(0, 2, 1)
            det = np.linalg.det(G)
            with np.errstate(divide="ignore", invalid="ignore"):
                gate.append(np.where(det > 0, np.trace(G, axis1=1, axis2=2) ** K / det, np.inf))
    r.gate = np.stack(gate, axis=1)
    r.scale = np.maximum(np.abs(terms).max(axis=(1, 2)), np.abs(dq_ref).max(axis=1))
    # ---- what kappa * scale leaves out (module docstring): in units of eps_T, before the max_dq clamp
    mv = lambda A, v: (A @ v[:, :, None])[:, :, 0]
    nrm = lambda v: np.linalg.norm(v, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        fx = (nrm(tgt[:, :3]) + nrm(tgt[:, :3] - dx0)) * np.minimum(1.0, lim["dx"] / size["dx"])
        fr = 4.0 * np.minimum(1.0, lim["dr"] / size["dr"])
    fx, fr = np.nan_to_num(fx, nan=0.0), np.nan_to_num(fr, nan=4.0)
    if method == 1:
        res = nrm(np.concatenate([dx, dr], axis=1) - mv(J, terms[:, 0]))
        extra = (r.kappa * res + fx + fr) / smin[0]
    elif method == 2:
        sj = np.linalg.svd(J, compute_uv=False)
        g = (sj / (sj * sj + 0.001)).max(axis=1)
        rhs = np.concatenate([dx, 0.3 * dr], axis=1)
        x = np.linalg.solve(blocks(J, 2)[0], rhs[:, :, None])[:, :, 0]
        extra = g * (r.sv[0].max(axis=1) * nrm(x) + fx + fr)
    else:
        rx, rw = nrm(dx - mv(J[:, :3], terms[:, 0])), nrm(dr - mv(J[:, 3:], terms[:, 1]))
        extra = (r.kappa * rx + fx) / smin[0] + (r.kappa * rw + fr) / smin[1]
    m = size["dq"]
    r.extra = extra * np.where(m > lim["dq"], lim["dq"] / np.where(m > 0, m, 1.0), 1.0)
    return r


def counted(r, dtype):
    dt = np.dtype(dtype)
    gate = KAPPA_GATE_DAMPED_F32 if (r.method == 2 and dt == F32) else KAPPA_GATE[dt]
    return (r.kappa <= gate) & ~r.near_cut & (r.w >= W_GATE[dt]) & (r.near_limit >= CLAMP_BAND[dt])


def bar(r, dtype, c=C):
    return c * eps(dtype) * (r.kappa * r.scale + r.extra)


def ratio(r, vp, dtype):
    """error of a step vp [B,n] over its bar, per row"""
    return np.abs(np.asarray(vp, dtype=np.float64) - r.dq_ref).max(axis=1) / bar(r, dtype)


def numpy_needs(r, dtype, issue_formula=False):
    """what numpy_step in `dtype` needs of the bar's constant on every row (to be read on the counted ones);
    issue_formula: of the constant of  C eps kappa scale  alone, without the residual and forward-kinematics terms"""
    dq, _, _ = numpy_step(_round(r.J, dtype), _round(r.dx, dtype), _round(r.dr, dtype), r.method, r.lim["dq"], dtype)
    err = np.abs(dq.astype(np.float64) - r.dq_ref).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return err / (eps(dtype) * r.kappa * r.scale) if issue_formula else C * ratio(r, dq, dtype)


def teacher_forced(tab, p, pp, tgt):
    """one oracle step from each stored position pp[:, t] of a path [B,T,n] -> the one_step namespace with every array
    of leading shape [B * T] (row-major: pair (b, t) at b * T + t)"""
    B, T, n = pp.shape
    return one_step(tab, p, np.asarray(pp, dtype=np.float64).reshape(B * T, n), np.repeat(np.asarray(tgt, dtype=np.float64), T, axis=0))


class Clamps:
    """which sides of the three clamps a case has seen on the reference, over all its runs"""

    def __init__(self):
        self.seen = {k: set() for k in ("dx", "dr", "dq")}

    def add(self, r):
        for k in self.seen:
            self.seen[k] |= set(np.unique(getattr(r, "clamp_" + k)).tolist())

    def check(self, what):
        for k, v in self.seen.items():
            assert v == {False, True}, f"{what}: the {k} clamp was only seen {'engaged' if True in v else 'not engaged'}"


def check_cap(r, dtype, rows, what, log=print):
    """the share of the random-posture pairs `rows` that is left out, asserted on the reference alone"""
    ok = counted(r, dtype)[rows]
    share = 1.0 - ok.mean()
    log(f"{what}: {share * 100:.1f} % of {ok.size} pairs left out")
    assert (~ok).sum() <= CAP * ok.size + 1e-9, f"{what}: {share * 100:.1f} % of the pairs are left out (cap {CAP * 100:.0f} %)"
    return share


def check_steps(r, vp, dtype, what, rows=None, log=print):
    """every counted pair of `rows` (default: all) within the bar -> worst error / bar"""
    ok = counted(r, dtype) & (True if rows is None else rows)
    rat = ratio(r, vp, dtype)
    worst = float(rat[ok].max()) if ok.any() else 0.0
    log(f"{what}: worst error / bar {worst:.3g} over {int(ok.sum())} counted pairs")
    bad = np.flatnonzero(ok & ~(rat <= 1))
    assert bad.size == 0, f"{what}: pairs {bad[:8].tolist()} miss the bar by {rat[bad[:8]].tolist()} (kappa {r.kappa[bad[:8]].tolist()})"
    return worst


def check_properties(q, pp, vp, p, dtype):
    """what holds on every row, singular ones included: finite, clamped, pp[t + 1] = pp[t] + vp[t] formed in dtype and
    pp[0] the input, bit for bit"""
    dt = np.dtype(dtype)
    assert pp.dtype == dt and vp.dtype == dt
    assert np.all(np.isfinite(pp)) and np.all(np.isfinite(vp))
    assert np.abs(vp).max(initial=0.0) <= p.max_dq * p.dt * (1 + 4 * eps(dt))
    if pp.shape[1]:
        assert np.array_equal(pp[:, 0], np.asarray(q, dtype=dt))
        assert np.array_equal(pp[:, 1:], pp[:, :-1] + vp[:, :-1])


# ---------------------------------------------------------------- the cases, shared by the host and the device tests
def arm_table(arm_id):
    """built-in names; synth<n>: tests/synthetic_arms.make_arm(n, 70 + n); ur5_rt: the UR5's table as a user arm;
    ur5_compiled, synthetic4_compiled: the tables whose plugins the build compiles (tests/compiled_*arms.py)"""
    if arm_id.startswith("synth") and arm_id[5:].isdigit():
        return synthetic(int(arm_id[5:]))
    if arm_id == "ur5_rt":
        return _abi.load_table("ur5")
    if arm_id == "ur5_compiled":
        from tests import compiled_plant_arms

        return compiled_plant_arms.table()
    if arm_id == "synthetic4_compiled":
        from tests import compiled_arms

        return compiled_arms.test_arms()["synthetic4"]
    return _abi.load_table(arm_id)


@functools.lru_cache(maxsize=None)
def one_step_case(arm_id, B, seed, dtype_name, method, limits=("default", "wide", "slow")):
    """the random draw of a case and its reference under each limit set, computed once -> (q, target, block, {set: ref})"""
    tab = arm_table(arm_id)
    q, tgt, block = draw_random(tab, B, seed, dtype_name)
    return q, tgt, block, {lim: one_step(tab, params(lim, method), q, tgt) for lim in limits}


def run_one_step(run, arm_id, dtype, method, B, seed, clamps=None, log=print):
    """`run(params, q, target) -> (pp, vp)` is the code under test.  The cap on the reference first, then per limit set
    the properties on every row and the bar on every counted pair (float32: outside the singular block, where the
    reference's formula itself carries no accuracy in that dtype) -> {set: worst error / bar}"""
    dt = np.dtype(dtype)
    q, tgt, block, refs = one_step_case(arm_id, B, seed, dt.name, method)
    what = f"{arm_id} {dt.name} method {method} B={B}"
    for lim, r in refs.items():
        check_cap(r, dt, block != 0, f"{what} {lim}", log)
    worst = {}
    for lim, r in refs.items():
        p = params(lim, method)
        pp, vp = run(p, q.astype(dt), tgt.astype(dt))
        check_properties(q, pp, vp, p, dt)
        worst[lim] = check_steps(r, vp[:, 0], dt, f"{what} {lim}", (block != 0) if dt == F32 else None, log)
        if clamps is not None:
            clamps.add(r)
    return worst


@functools.lru_cache(maxsize=None)
def path_case(arm_id, B, T, seed, dtype_name, method, limits):
    """a reachable draw, the oracle's own path from it and that path's teacher-forced reference (for the cap)"""
    tab = arm_table(arm_id)
    q0, tgt = draw_reachable(tab, B, seed, dtype_name)
    p = params(limits, method, T)
    pp, vp = O.ik_paths(tab, p, q0, tgt)
    return q0, tgt, pp, vp, teacher_forced(tab, p, _round(pp, dtype_name), tgt)


def run_path(run, arm_id, dtype, method, B, T, seed, limits, clamps=None, log=print, free_running=False):
    """every stored step of the path of the code under test against one oracle step from the path's own position;
    free_running (float64, to be asked under the default limits: with steps of 5 cm and 0.3 rad the wide ones make
    the iteration sensitive to rounding, two float64 evaluations part by up to 0.7 rad within 40 steps while every step
    meets its bar): the rows without an uncounted step within 1e-8 of the oracle's own path as well"""
    dt = np.dtype(dtype)
    q0, tgt, pp_o, vp_o, r_o = path_case(arm_id, B, T, seed, dt.name, method, limits)
    what = f"{arm_id} {dt.name} method {method} B={B} T={T} {limits}"
    check_cap(r_o, dt, np.ones(B * T, dtype=bool), what + " (oracle's path)", log)
    p = params(limits, method, T)
    pp, vp = run(p, q0.astype(dt), tgt.astype(dt))
    check_properties(q0, pp, vp, p, dt)
    r = teacher_forced(arm_table(arm_id), p, pp, tgt)
    if clamps is not None:
        clamps.add(r)
    worst = check_steps(r, vp.reshape(B * T, -1), dt, what, None, log)
    if free_running and dt == F64:
        rows = counted(r, dt).reshape(B, T).all(axis=1) & counted(r_o, dt).reshape(B, T).all(axis=1)
        d = max(np.abs(pp - pp_o)[rows].max(initial=0.0), np.abs(vp - vp_o)[rows].max(initial=0.0))
        log(f"{what}: free-running path within {d:.3g} of the oracle's on {int(rows.sum())} rows")
        assert rows.sum() >= B // 2 and d < 1e-8
    return worst


# ---------------------------------------------------------------- rows next to a singularity
def _kappa3(o, q):
    J = np.array([o.J("EE", qb) for qb in q]).reshape(len(q), 6, o.n)
    sx, sw = np.linalg.svd(J[:, :3], compute_uv=False), np.linalg.svd(J[:, 3:], compute_uv=False)
    return sx[:, 0] / sx[:, -1] + sw[:, 0] / sw[:, -1]


@functools.lru_cache(maxsize=None)
def draw_ill(arm_id, B, seed, dtype_name, lo=200.0, hi=700.0):
    """postures whose method-3 kappa lies in lo .. hi: each a point of a random line through joint space, found by
    bisection between a well-conditioned point and the worst one of a grid, with random targets -> (q, target).  In
    float32 such rows count (kappa <= 1e3) and sit far beyond pinv_KxN's gate, where J^T (J J^T)^-1 would lose
    eps kappa^2 = 1e-3 .. 3e-2 of the step: they pass only through the Jacobi fallback.  For arms whose blocks are
    square or nearly so (three, four joints): a random line crosses their singularities; a 3 x 6 block is rarely singular."""
    tab = arm_table(arm_id)
    o, n, r = O.Oracle(tab), tab["n_joints"], np.random.RandomState(seed)
    rows, s = [], np.linspace(0, 3, 301)
    for _ in range(50 * B):  # about one line in three crosses a singularity closely enough
        if len(rows) == B:
            break
        q0, d = r.uniform(-3, 3, n), r.normal(size=n)
        d /= np.linalg.norm(d)
        k = _kappa3(o, q0 + s[:, None] * d)
        i = int(np.argmax(k))
        j, step = i, (-1 if i > 0 else 1)
        while 0 <= j + step < len(s) and k[j] >= lo:
            j += step
        if k[i] < lo or k[j] >= lo:
            continue
        a, b = s[j], s[i]  # kappa(a) < lo <= kappa(b)
        for _ in range(40):
            m = 0.5 * (a + b)
            q = _round(q0 + m * d, dtype_name)
            km = _kappa3(o, q[None])[0]
            if lo <= km <= hi:
                rows.append(q)
                break
            a, b = (m, b) if km < lo else (a, m)
    assert len(rows) == B
    q = np.array(rows)
    tgt = _round(np.hstack([r.uniform(-0.5, 0.5, (B, 3)), r.uniform(-3, 3, (B, 3))]), dtype_name)
    return q, tgt


def run_ill(run, arm_id, dtype, B, seed, log=print):
    """method 3 on draw_ill's rows under the default and the wide limits: every row counts, none passes the float32 gate
    of the Cholesky path, all meet the bar -> worst error / bar.  Asked in float32 only: the float64 gate (1e6) does let
    such rows through, and there the Cholesky path's eps kappa^2 is up to 1.5 times this bar (profiles/ik_tests.md)"""
    dt = np.dtype(dtype)
    q, tgt = draw_ill(arm_id, B, seed, dt.name)
    worst = 0.0
    for lim in ("default", "wide"):
        p = params(lim, 3)
        r = one_step(arm_table(arm_id), p, q, tgt)
        ok = counted(r, dt)
        assert ok.mean() >= 0.9 and r.kappa[ok].min() >= 150 and not (r.gate < FAST_GATE[F32]).all(axis=1).any()
        pp, vp = run(p, q.astype(dt), tgt.astype(dt))
        check_properties(q, pp, vp, p, dt)
        worst = max(worst, check_steps(r, vp[:, 0], dt, f"{arm_id} {dt.name} next to a singularity, {lim}", None, log))
    return worst
