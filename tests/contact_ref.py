"""Reference of the end-effector contact (include/abrk.h, abrk_contact_step_batch), restated in NumPy on the oracle's
Tx, J and R with x= : for row b, with p = Tx(frame, q, x=off), Jp = J(frame, q, x=off)[:3], v = Jp dq and every surface
(n, d, k, c, mu, rho) of the row
    delta = d + rho - n.p;  vn = n.v;  fn = max(0, k delta - c vn) where delta > 0, else 0
    f = fn n - mu fn vt / sqrt(|vt|^2 + vs^2),  vt = v - vn n
    tau = Jp^T sum f;  report = [F, R(frame, q)^T F, max delta, #(delta > 0)]
Shared by the CPU and the GPU tests, which feed it inputs already rounded to the dtype under test (rounded()).

Inputs (draw_case): states of plant_fx_ref.draw; surfaces placed relative to each row's own reference p so that every
branch is populated by construction - row b presses (b % 3 == 0), is clear of every surface (1) or presses while leaving
fast enough that k delta - c vn < 0 (2).  |delta| in 10 - 40 mm, k in 5e3 - 5e4 N/m, c in 50 - 500 N s/m, mu in 0 - 1, rho
in 0 - 20 mm, normals uniform on the sphere; a draw of (n, delta, k, c) is repeated until the surface sits on its side of
the switch with the margin MARGIN.  Further surfaces of a pressing row take any branch, those of the other rows a branch
without force, so that `tau` of a row without force is exactly zero.

Which rows count.  fn = k delta - c vn is a difference: where it cancels, the error of delta is magnified by
k delta / |k delta - c vn|.  The fp32 forward kinematics is good to a few 1e-7 m at a 1 m reach, i.e. delta of 10 mm
carries about 3e-5 relative error; the bar on tau is 1e-4, and half of it is left to the other fp32 roundings (Jacobian,
velocity, friction, the sum over surfaces).  So in fp32 a surface is trusted while |k delta - c vn| >= 0.6 k delta
(3e-5 / 0.6 = 5e-5), and a row with a penetrated surface below that is left out; in fp64 the same reasoning with 1e-15 in
place of 3e-5 leaves a band of 1e-9 with room to spare.  A case may leave out CAP rows: none in fp64, one in fp32.  The
generator's MARGIN of 0.75 is above both bands, so the seeds used leave out no row; the tests assert that on the
reference, together with the branch counts."""
import numpy as np

from oracle.oracle import Oracle
from tests.plant_fx_ref import TOL_F32, TOL_F64, draw, rel_err, rounded  # noqa: F401  (re-exported to the tests)

BAND = {np.dtype(np.float64): 1e-9, np.dtype(np.float32): 0.6}
CAP = {np.dtype(np.float64): 0, np.dtype(np.float32): 1}
MARGIN = 0.75
VS = 1e-3
PRESS, CLEAR, LEAVE = 0, 1, 2


def tol_of(dtype):
    return TOL_F64 if np.dtype(dtype) == np.float64 else TOL_F32


def surface_force(s, p, v, vs):
    """one surface (8 values) on the tip at p moving with v -> (f [3], delta, margin); margin = |k delta - c vn| /
    (k delta) of a penetrated surface, inf of a clear one"""
    n, d, k, c, mu, rho = s[:3], s[3], s[4], s[5], s[6], s[7]
    delta = d + rho - n @ p
    if delta <= 0:
        return np.zeros(3), delta, np.inf
    vn = n @ v
    push = k * delta - c * vn
    fn = max(0.0, push)
    vt = v - vn * n
    f = fn * n - mu * fn * vt / np.sqrt(vt @ vt + vs * vs)
    return f, delta, abs(push) / (k * delta)


class ContactRef:
    """the law for one arm table; frame, off, vs as the entry point takes them"""

    def __init__(self, table, frame="EE", off=(0, 0, 0), vs=VS):
        self.O = Oracle(table)
        self.n = int(table["n_joints"])
        self.frame, self.off, self.vs = frame, np.asarray(off, dtype=np.float64), float(vs)

    def point(self, q):
        """-> p [3], Jp [3, n]"""
        return self.O.Tx(self.frame, q, x=self.off), self.O.J(self.frame, q, x=self.off)[:3]

    def step(self, q, dq, surface):
        """q, dq [B, n], surface [B, S, 8] (float64) -> tau [B, n], report [B, 8], margin [B]: the smallest margin of
        the row's penetrated surfaces"""
        B, S = surface.shape[0], surface.shape[1]
        tau, rep, margin = np.zeros((B, self.n)), np.zeros((B, 8)), np.full(B, np.inf)
        for b in range(B):
            p, Jp = self.point(q[b])
            v = Jp @ dq[b]
            F, deltas = np.zeros(3), []
            for s in range(S):
                f, delta, m = surface_force(surface[b, s], p, v, self.vs)
                F += f
                deltas.append(delta)
                margin[b] = min(margin[b], m)
            tau[b] = Jp.T @ F
            rep[b, 0:3] = F
            rep[b, 3:6] = self.O.R(self.frame, q[b]).T @ F
            rep[b, 6] = max(deltas)
            rep[b, 7] = sum(d > 0 for d in deltas)
        return tau, rep, margin


def _unit(r):
    x = r.normal(size=3)
    return x / np.linalg.norm(x)


V_LEAVE = 0.25  # a point slower than this cannot leave fast enough inside the ranges above: its row is a clear one


def _draw_surface(r, what, v):
    """-> n, delta, k, c of one surface on branch `what` for a tip moving with v.  The normal is uniform on the sphere
    (on the half with n.v > 0 for a leaving surface); delta, k and c are uniform over the part of their ranges that
    puts the surface on its side of the switch with MARGIN to spare."""
    for _ in range(10000):
        n = _unit(r)
        vn = n @ v
        if what == CLEAR:
            return n, -r.uniform(0.01, 0.04), r.uniform(5e3, 5e4), r.uniform(50, 500)
        if what == PRESS:
            delta, k = r.uniform(0.01, 0.04), r.uniform(5e3, 5e4)
            c_max = 500.0 if vn <= 0 else min(500.0, (1 - MARGIN) * k * delta / vn)  # c vn <= (1 - MARGIN) k delta
            if c_max > 50:
                return n, delta, k, r.uniform(50, c_max)
            continue
        if vn < 0:
            n, vn = -n, -vn
        push_max = 500.0 * vn / (1 + MARGIN)  # k delta <= c vn / (1 + MARGIN) with c <= 500
        if push_max <= 5e3 * 0.01:
            continue
        delta = r.uniform(0.01, min(0.04, push_max / 5e3))
        k = r.uniform(5e3, min(5e4, push_max / delta))
        return n, delta, k, r.uniform(max(50.0, (1 + MARGIN) * k * delta / vn), 500)
    raise AssertionError(f"no draw reaches branch {what} (|v| = {np.linalg.norm(v):.3g})")


def draw_surfaces(seed, ref, q, dq, S):
    """-> surface [B, S, 8] (float64), kind [B] of PRESS / CLEAR / LEAVE"""
    r = np.random.RandomState(seed)
    B = q.shape[0]
    kind = np.arange(B) % 3
    out = np.zeros((B, S, 8))
    for b in range(B):
        p, Jp = ref.point(q[b])
        v = Jp @ dq[b]
        if kind[b] == LEAVE and np.linalg.norm(v) < V_LEAVE:
            kind[b] = CLEAR
        for s in range(S):
            if s == 0:
                what = kind[b]
            elif kind[b] == PRESS:
                what = r.randint(3) if np.linalg.norm(v) >= V_LEAVE else r.randint(2)
            else:
                what = CLEAR if kind[b] == CLEAR else (CLEAR, LEAVE)[r.randint(2)]
            n, delta, k, c = _draw_surface(r, what, v)
            mu, rho = r.uniform(0, 1), r.uniform(0, 0.02)
            out[b, s] = [*n, n @ p + delta - rho, k, c, mu, rho]
    return out, kind


_cases = {}


def draw_case(table, name, frame, off, S, B, dtype, seed):
    """-> dict(q, dq, surface (rounded to dtype, float64), ref, tau, report, keep [B], kind [B]).  Computed once per
    key and shared: do not write into it.  Asserts the populations and the cap on the reference."""
    key = (name, frame, tuple(off), S, B, np.dtype(dtype).name, seed)
    if key in _cases:
        return _cases[key]
    n = int(table["n_joints"])
    dt_ = np.dtype(dtype)
    ref = ContactRef(table, frame, off)
    q, dq = draw(seed, B, n)[:2]
    q, dq = rounded(dtype, q, dq)
    surface, kind = draw_surfaces(seed + 1000, ref, q, dq, S)
    surface = rounded(dtype, surface)[0]  # (|n| stays 1 to the type's rounding: inside the entry's 1e-6)
    tau, rep, margin = ref.step(q, dq, surface)
    keep = margin >= BAND[dt_]
    assert (~keep).sum() <= CAP[dt_], (key, int((~keep).sum()))
    # the branches, read off the reference alone: a force; no penetration; penetration without force
    force = np.abs(rep[:, :3]).max(axis=1) > 0
    pressing, clear, leaving = force, rep[:, 7] == 0, (rep[:, 7] > 0) & ~force
    if B >= 30:
        for pop in (pressing, clear, leaving):
            assert pop.sum() >= B / 10, (key, int(pressing.sum()), int(clear.sum()), int(leaving.sum()))
    assert np.array_equal(pressing, kind == PRESS) and np.array_equal(clear, kind == CLEAR)
    _cases[key] = dict(q=q, dq=dq, surface=surface, ref=ref, tau=tau, report=rep, keep=keep, kind=kind,
                       pressing=pressing)
    return _cases[key]


def check(case, tau, report, dtype, what=""):
    """tau and report of the code under test against the case's reference -> the worst error found (asserted <= bar)"""
    tol = tol_of(dtype)
    on = case["pressing"] & case["keep"]
    off = ~case["pressing"]
    assert np.isfinite(tau).all() and np.isfinite(report).all()
    assert not tau[off].any(), f"{what}: a row without force has tau != 0"
    assert not report[off, :6].any(), f"{what}: a row without force reports one"
    worst = 0.0
    if on.any():
        e_tau = rel_err(tau[on], case["tau"][on])
        e_f = rel_err(report[on, 0:3], case["report"][on, 0:3])
        e_l = rel_err(report[on, 3:6], case["report"][on, 3:6])
        print(f"{what}: tau {e_tau:.2e} force {e_f:.2e} force_local {e_l:.2e} (left out {int((~case['keep']).sum())})")
        assert e_tau <= tol and e_f <= tol and e_l <= tol, (what, e_tau, e_f, e_l)
        worst = max(e_tau, e_f, e_l)
    # depth to the fp32 / fp64 kinematics (absolute: a few 1e-7 m at a 1 m reach in fp32), the count exactly
    dd = np.abs(report[:, 6] - case["report"][:, 6]).max()
    assert dd <= (1e-12 if np.dtype(dtype) == np.float64 else 2e-6), (what, dd)
    assert np.array_equal(report[:, 7], case["report"][:, 7]), what
    return worst
