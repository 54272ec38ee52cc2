"""Reference of the force-control law (include/abrk.h, abrk_force_control_batch), restated in NumPy on the oracle's Tx, J
with x=, M and g: for row b, with p = Tx(frame, q, x=off), Jp = J(frame, q, x=off)[:3], v = Jp dq
    A    = Jp M^-1 Jp^T;   Mx = inv(A) where det(A) > 1e-3, else pinv(A, rcond=1e-4)
    a    = kp (x_d - p) + kv (v_d - v);   a_n = n.a;   v_n = n.v;   f_m = n.F
    f_m > f_touch:  e = f_des - f_m;  I' = clamp(I + ki e dt, +-i_max);  F_c = Mx (a - a_n n - kvf v_n n) - (f_des + kf e + I') n
    otherwise:      I' = 0;                                              F_c = Mx (a - a_n n + kv (-v_app - v_n) n)
    u    = Jp^T F_c - [use_g] g - kv_null (M dq - Jp^T Mx v)
Shared by the CPU and the GPU tests, which feed it inputs and gains already rounded to the dtype under test (rounded()).

Inputs (draw_case): states of plant_fx_ref.draw; x_d within 0.1 m of each row's own p, v_d in +-0.5 m/s, normals uniform
on the sphere (planar arms: projected into the x-y plane and normalised - there A has rank 2 and every row takes the pinv
branch), f_des in 1 - 40 N.  Rows fall into three populations by b % 3:
  pressing    F = f n + a tangential part of up to 5 N, f in 2 - 30 N (f_touch = 0.5), integ in +-1
  free        F = 0 exactly, integ = 0.7
  saturating  pressing, with integ 10 - 90 % of |ki e dt| inside +-i_max and e signed so that the clamp acts
No row sits on a switch: f_m is outside [0.5 f_touch, 2 f_touch] by construction (>= 2 N or 0), and the pre-clamp
integral is at least 10 % of ki e dt away from +-i_max.  Two more margins keep the fp32 bar meaningful on `integ`, whose
"row" is one number: |e| >= 1 N (f_des is redrawn), so that ki e dt is a few thousand fp32 roundings of the integral it
is added to, and |I + ki e dt| >= 0.05 on the pressing rows (integ is redrawn): the sum of two fp32 numbers of size 1
carries an absolute error of 1e-7, which the bar of 1e-4 allows down to 1e-3.

Which rows count.  With s the singular values of the reference's A, a row is left out if some s_i / s_max lies in
[1e-5, 1e-3]: it is within a factor 10 of the rcond cut, where the other arithmetic may truncate differently, or the kept
part has cond >= 1e3, the gate tests/cases.py uses for three task rows in fp32.  The same rule for both dtypes.  A case
may leave out 5 % of its rows; the tests assert that on the reference alone, together with the three populations."""
import numpy as np

from oracle.oracle import Oracle
from tests.plant_fx_ref import TOL_F32, TOL_F64, draw, rel_err, rounded  # noqa: F401  (re-exported to the tests)

GAINS = dict(kp=100.0, kv=20.0, kf=0.5, ki=20.0, i_max=50.0, kvf=20.0, f_touch=0.5, v_app=0.05, kv_null=10.0)
DT = 1e-3
OFFSET = (0.03, -0.02, 0.11)
SEED = 71
LEFT_OUT = (1e-5, 1e-3)
CAP_FRACTION = 0.05
PRESS, FREE, SATURATE = 0, 1, 2


def tol_of(dtype):
    return TOL_F64 if np.dtype(dtype) == np.float64 else TOL_F32


def gains_rounded(dtype, gains, dt):
    """the gains and dt as the kernel holds them: rounded to `dtype`"""
    r = lambda x: float(np.asarray(x, dtype=dtype))  # noqa: E731
    return {k: r(v) for k, v in gains.items()}, r(dt)


class ForceRef:
    """the law for one arm table; frame, off, gains, dt, use_g as the entry point takes them"""

    def __init__(self, table, frame="EE", off=(0, 0, 0), gains=GAINS, dt=DT, use_g=True):
        self.O = Oracle(table)
        self.n = int(table["n_joints"])
        self.frame, self.off, self.dt, self.use_g = frame, np.asarray(off, dtype=np.float64), float(dt), bool(use_g)
        self.g = dict(gains)

    def point(self, q):
        """-> p [3], Jp [3, n]"""
        return self.O.Tx(self.frame, q, x=self.off), self.O.J(self.frame, q, x=self.off)[:3]

    def row(self, q, dq, xd, vd, cmd, F, integ):
        """-> u [n], the new integral, the singular values of A [3], det(A)"""
        G = self.g
        p, Jp = self.point(q)
        M = self.O.M(q)
        A = Jp @ np.linalg.inv(M) @ Jp.T
        det = np.linalg.det(A)
        Mx = np.linalg.inv(A) if det > 1e-3 else np.linalg.pinv(A, rcond=1e-4)
        v = Jp @ dq
        n, f_des = cmd[:3], cmd[3]
        a = G["kp"] * (xd - p) + G["kv"] * (vd - v)
        a_n, v_n, f_m = n @ a, n @ v, n @ F
        if f_m > G["f_touch"]:
            e = f_des - f_m
            integ = min(max(integ + G["ki"] * e * self.dt, -G["i_max"]), G["i_max"])
            Fc = Mx @ (a - a_n * n - G["kvf"] * v_n * n) - (f_des + G["kf"] * e + integ) * n
        else:
            integ = 0.0
            Fc = Mx @ (a - a_n * n + G["kv"] * (-G["v_app"] - v_n) * n)
        u = Jp.T @ Fc - G["kv_null"] * (M @ dq - Jp.T @ (Mx @ v))
        if self.use_g:
            u = u - self.O.g(q)
        return u, integ, np.linalg.svd(A, compute_uv=False), det

    def step(self, q, dq, target, tv, cmd, force, integ):
        """q, dq [B, n], target [B, 6], tv [B, 6] or None, cmd [B, 4], force [B, >= 3], integ [B] (float64) -> u [B, n],
        integ [B], s [B, 3], det [B]"""
        B = q.shape[0]
        u, I, s, det = np.zeros((B, self.n)), np.zeros(B), np.zeros((B, 3)), np.zeros(B)
        for b in range(B):
            vd = np.zeros(3) if tv is None else tv[b, :3]
            u[b], I[b], s[b], det[b] = self.row(q[b], dq[b], target[b, :3], vd, cmd[b], force[b, :3], integ[b])
        return u, I, s, det


def counted(s):
    """s [B, 3] singular values of A -> keep [B]: no s_i / s_max inside LEFT_OUT"""
    ratio = s / s.max(axis=1, keepdims=True)
    return ~((ratio >= LEFT_OUT[0]) & (ratio <= LEFT_OUT[1])).any(axis=1)


def _unit(r, planar):
    while True:
        x = r.normal(size=3)
        if planar:
            x[2] = 0.0
        if np.linalg.norm(x) > 1e-3:
            return x / np.linalg.norm(x)


def draw_inputs(seed, ref, q, dtype, planar, gains=GAINS, dt=DT):
    """-> target [B, 6], tv [B, 6], cmd [B, 4], force [B, 3], integ [B] (rounded to dtype, float64), kind [B]"""
    r = np.random.RandomState(seed)
    B = q.shape[0]
    kind = np.arange(B) % 3
    target, tv = r.uniform(-1, 1, (B, 6)), r.uniform(-0.5, 0.5, (B, 6))
    cmd, force, integ = np.zeros((B, 4)), np.zeros((B, 3)), np.zeros(B)
    for b in range(B):
        target[b, :3] = ref.point(q[b])[0] + r.uniform(-0.1, 0.1, 3)
        n = rounded(dtype, _unit(r, planar))[0]
        if kind[b] == FREE:
            cmd[b], integ[b] = [*n, r.uniform(1, 40)], 0.7
            continue
        t = r.uniform(-5, 5, 3)
        F = rounded(dtype, r.uniform(2, 30) * n + (t - (t @ n) * n))[0]
        f_m = n @ F
        assert f_m > 2 * gains["f_touch"]
        for _ in range(1000):
            f_des = rounded(dtype, r.uniform(1, 40))[0]
            step = gains["ki"] * (f_des - f_m) * dt
            if abs(f_des - f_m) < 1:
                continue
            if kind[b] == PRESS:
                I = rounded(dtype, r.uniform(-1, 1))[0]
                if abs(I + step) < 0.05:
                    continue
            else:  # 10 - 90 % of the step inside the bound it is heading for
                I = rounded(dtype, np.sign(step) * (gains["i_max"] - r.uniform(0.1, 0.9) * abs(step)))[0]
                if abs(I + step) < gains["i_max"] + 0.1 * abs(step) or abs(I) > gains["i_max"] - 0.1 * abs(step):
                    continue
            break
        else:
            raise AssertionError(f"row {b}: no draw with the margins")
        cmd[b], force[b], integ[b] = [*n, f_des], F, I
    target, tv = rounded(dtype, target, tv)
    return target, tv, cmd, force, integ, kind


_cases = {}


def draw_case(table, name, frame, off, B, dtype, seed=SEED, gains=GAINS, dt=DT, use_g=True, with_tv=True):
    """-> dict(q, dq, target, tv, cmd, force, integ (rounded to dtype, float64), ref, u, integ_new, keep [B], kind [B],
    gains, dt (rounded)).  Computed once per key and shared: do not write into it.  Asserts the populations and the cap
    on the reference."""
    key = (name, frame, tuple(off), B, np.dtype(dtype).name, seed, tuple(sorted(gains.items())), dt, use_g, with_tv)
    if key in _cases:
        return _cases[key]
    n = int(table["n_joints"])
    g, h = gains_rounded(dtype, gains, dt)
    ref = ForceRef(table, frame, off, g, h, use_g)
    q, dq = draw(seed, B, n)[:2]
    q, dq = rounded(dtype, q, dq)
    planar = name in ("twojoint", "threejoint")
    target, tv, cmd, force, integ, kind = draw_inputs(seed + 1000, ref, q, dtype, planar, g, h)
    if not with_tv:
        tv = None
    u, I, s, det = ref.step(q, dq, target, tv, cmd, force, integ)
    keep = counted(s)
    assert (~keep).sum() <= CAP_FRACTION * B, (key, int((~keep).sum()))
    # the populations, read off the reference alone
    f_m = (cmd[:, :3] * force).sum(axis=1)
    touching = f_m > g["f_touch"]
    assert not ((f_m >= 0.5 * g["f_touch"]) & (f_m <= 2 * g["f_touch"])).any()
    clamped = touching & (np.abs(I) == g["i_max"])
    pressing, free = touching & ~clamped, ~touching
    if B >= 30:
        for pop in (pressing, free, clamped):
            assert pop.sum() >= B / 10, (key, int(pressing.sum()), int(free.sum()), int(clamped.sum()))
    assert np.array_equal(pressing, kind == PRESS) and np.array_equal(free, kind == FREE)
    assert not I[free].any()
    _cases[key] = dict(q=q, dq=dq, target=target, tv=tv, cmd=cmd, force=force, integ=integ, ref=ref, u=u, integ_new=I,
                       keep=keep, kind=kind, gains=g, dt=h, s=s, det=det, free=free, clamped=clamped)
    return _cases[key]


def check(case, u, integ, dtype, what="", rows=None, u_ref=None, integ_ref=None):
    """u and the new integral of the code under test against the case's reference (rows: a slice of the case; u_ref,
    integ_ref: another reference for the same rows) -> the worst errors (u, integ), asserted <= the bar"""
    rows = slice(None) if rows is None else rows
    tol = tol_of(dtype)
    u_ref = case["u"][rows] if u_ref is None else u_ref
    integ_ref = case["integ_new"][rows] if integ_ref is None else integ_ref
    keep, free = case["keep"][rows], case["free"][rows]
    assert np.isfinite(u).all() and np.isfinite(integ).all(), f"{what}: a row is not finite"
    assert not integ[free].any(), f"{what}: the integral of a free row is not exactly 0"
    if not keep.any():
        return 0.0, 0.0
    e_u = rel_err(u[keep], u_ref[keep])
    on = keep & ~free
    e_i = rel_err(integ[on][:, None], integ_ref[on][:, None]) if on.any() else 0.0
    print(f"{what}: u {e_u:.2e} integ {e_i:.2e} (left out {int((~keep).sum())})")
    assert e_u <= tol and e_i <= tol, (what, e_u, e_i)
    return e_u, e_i
