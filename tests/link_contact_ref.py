"""Reference of the whole-arm contact (include/abrk.h, abrk_link_contact_step_batch), restated in NumPy on the oracle's
T, Tx and J with x= : segment i runs from a_i = Tx("joint{i}") to b_i = Tx("joint{i+1}") (Tx("EE") for the last one) and
is a body of link i+1; for every (obstacle, segment) pair, obstacle-major and segment-minor,
    t = clamp((c - a).(b - a) / |b - a|^2, 0, 1);  x = a + t (b - a);  e = x - c;  d = |e|;  delta = R + r_i - d
    n = e / d;  v = Jx dq with Jx = J("link{i+1}", q, x=m)[:3], m = solve(R_link, x - o_link)
    vn = n.v;  fn = max(0, k delta - c vn) where delta > 0;  vt = v - vn n;  f = fn n - mu fn vt / sqrt(|vt|^2 + vs^2)
    tau += Jx^T f
(`solve`, not the transpose: Jaco2's rounded rotation constants are not orthogonal.)
report = [sum f, the deepest delta, #(delta > 0), segment, obstacle and t of the deepest pair (first on a tie)].
Shared by the CPU and the GPU tests, which feed it inputs already rounded to the dtype under test (rounded()).

Inputs (draw_case): states of plant_fx_ref.draw; radii 20 - 50 mm, one per segment; obstacles placed relative to each
row's own segments so that every branch is populated by construction.  Row b's first obstacle, by b % 6:
  IN (0) pushes a segment at 0.1 < t < 0.9;  CLEAR (1): the row is clear of everything;  LEAVE (2) penetrates while the
  point leaves fast enough that k delta - c vn < 0 - the row has no force;  T0 (3) / T1 (4) push a segment's end from
  beyond it, so that t clamps at 0 / 1;  TWO (5) sits at the joint two neighbouring segments share and penetrates both.
|delta| in 10 - 40 mm, R in 30 - 80 mm, k in 5e3 - 5e4 N/m, c in 50 - 500 N s/m, mu in 0 - 1 (the ranges of
contact_ref.py).  Further obstacles of a pushing row push or are clear, those of the other rows are clear, so that `tau`
of a row without force is exactly zero.  A sphere of that size near a joint also meets the neighbouring segments; a row's
draw is repeated until the whole row, every pair of it, is of its kind and holds the margins below.  A LEAVE row whose
arm is too slow to leave inside the ranges becomes a CLEAR one.

Which rows count (the reasoning of contact_ref.py).  fn = k delta - c vn is a difference; the fp32 kinematics is good to
a few 1e-7 m at a 1 m reach, so delta of 10 mm carries about 3e-5 relative error and a pair is trusted while
|k delta - c vn| >= 0.6 k delta (fp32; fp64: 1e-9).  A row with a penetrated pair below that is left out.  So is, for
the count and the three index columns, a row whose deepest pair leads the runner-up by less than DEPTH_BAND, or that has
a pair with |delta| below it (the count would flip): 5e-6 m in fp32 - ten times the kinematics' error - and 1e-11 m in
fp64.  A case may leave out CAP rows: none in fp64, one in fp32.  The generator keeps MARGIN = 0.75 on every penetrated
pair, 1e-4 m on every |delta| and on the lead: above all bands, so the seeds used leave out no row; the tests assert
that on the reference, together with the branch counts."""
import numpy as np

from oracle.oracle import Oracle
from tests.plant_fx_ref import TOL_F32, TOL_F64, draw, rel_err, rounded  # noqa: F401  (re-exported to the tests)

BAND = {np.dtype(np.float64): 1e-9, np.dtype(np.float32): 0.6}
DEPTH_BAND = {np.dtype(np.float64): 1e-11, np.dtype(np.float32): 5e-6}
CAP = {np.dtype(np.float64): 0, np.dtype(np.float32): 1}
MARGIN = 0.75
GAP = 1e-4  # the generator's margin on |delta| of every pair and on the lead of the deepest one (m)
VS = 1e-3
IN, CLEAR, LEAVE, T0, T1, TWO = range(6)
PUSHING = (IN, T0, T1, TWO)


def tol_of(dtype):
    return TOL_F64 if np.dtype(dtype) == np.float64 else TOL_F32


class LinkContactRef:
    """the law for one arm table; radius [n] (< 0: segment off), vs as the entry point takes them"""

    def __init__(self, table, radius, vs=VS):
        self.O = Oracle(table)
        self.n = int(table["n_joints"])
        self.radius = np.broadcast_to(np.asarray(radius, dtype=np.float64), (self.n,)).copy()
        self.vs = float(vs)

    def segments(self, q):
        """-> a [n,3], b [n,3]"""
        o = [self.O.Tx(f"joint{i}", q) for i in range(self.n)] + [self.O.Tx("EE", q)]
        return np.array(o[:-1]), np.array(o[1:])

    def jx(self, i, q, x):
        """the point Jacobian [3,n] of the material point of link i+1 that is at x"""
        T = self.O.T(f"link{i + 1}", q)
        m = np.linalg.solve(T[:3, :3], x - T[:3, 3])
        return self.O.J(f"link{i + 1}", q, x=m)[:3]

    def pairs(self, q, dq, obstacle, a=None, b=None):
        """one row, obstacle [K,7] -> the active pairs in loop order, each a dict(ob, seg, t, x, delta, f, Jx, margin);
        margin = |k delta - c vn| / (k delta) of a penetrated pair, inf of a clear one"""
        if a is None:
            a, b = self.segments(q)
        out = []
        for ob, s in enumerate(obstacle):
            c, R, k, cd, mu = s[:3], s[3], s[4], s[5], s[6]
            for i in range(self.n):
                vl = b[i] - a[i]
                len2 = vl @ vl
                if self.radius[i] < 0 or not len2 > 0:
                    continue
                t = min(1.0, max(0.0, (c - a[i]) @ vl / len2))
                x = b[i] if t == 1.0 else a[i] + t * vl
                e = x - c
                d = np.sqrt(e @ e)
                delta = R + self.radius[i] - d
                p = dict(ob=ob, seg=i, t=t, x=x, delta=delta, f=np.zeros(3), Jx=None, margin=np.inf)
                if delta > 0:
                    n = e / d if d > 0 else np.zeros(3)
                    p["Jx"] = self.jx(i, q, x)
                    v = p["Jx"] @ dq
                    vn = n @ v
                    push = k * delta - cd * vn
                    fn = max(0.0, push)
                    vt = v - vn * n
                    p["f"] = fn * n - mu * fn * vt / np.sqrt(vt @ vt + self.vs * self.vs)
                    p["fn"] = fn
                    p["margin"] = abs(push) / (k * delta)
                out.append(p)
        return out

    def row(self, q, dq, obstacle, a=None, b=None):
        """-> tau [n], report [8], margin, gap: the smallest margin of the row's penetrated pairs; the smaller of the
        deepest pair's lead over the runner-up and the smallest |delta|"""
        ps = self.pairs(q, dq, obstacle, a, b)
        tau, rep = np.zeros(self.n), np.zeros(8)
        if not ps:
            rep[3:] = [-np.inf, 0, -1, -1, 0]
            return tau, rep, np.inf, np.inf
        for p in ps:
            if p["Jx"] is not None:
                tau += p["Jx"].T @ p["f"]
                rep[:3] += p["f"]
        deltas = np.array([p["delta"] for p in ps])
        best = int(np.argmax(deltas))  # (the first on a tie)
        rep[3] = deltas[best]
        rep[4] = (deltas > 0).sum()
        rep[5], rep[6], rep[7] = ps[best]["seg"], ps[best]["ob"], ps[best]["t"]
        lead = np.inf if len(ps) == 1 else deltas[best] - np.delete(deltas, best).max()
        return tau, rep, min(p["margin"] for p in ps), min(lead, np.abs(deltas).min())

    def step(self, q, dq, obstacle):
        """q, dq [B,n], obstacle [B,K,7] (float64) -> tau [B,n], report [B,8], margin [B], gap [B]"""
        B = q.shape[0]
        tau, rep, margin, gap = np.zeros((B, self.n)), np.zeros((B, 8)), np.zeros(B), np.zeros(B)
        for r in range(B):
            tau[r], rep[r], margin[r], gap[r] = self.row(q[r], dq[r], obstacle[r])
        return tau, rep, margin, gap


def _unit(r):
    x = r.normal(size=3)
    return x / np.linalg.norm(x)


def _place(r, ref, a, b, what, sign, leave=None):
    """one obstacle [7] aimed at a segment on branch `what`; sign = +1: penetrating by 10 - 40 mm, -1: clear by that.
    leave = (q, dq): the obstacle lies where the segment's point comes from, and delta, k, c are uniform over the part
    of their ranges in which k delta - c vn < 0 with MARGIN to spare (None where the point is too slow for that)"""
    live = [i for i in range(ref.n) if ref.radius[i] >= 0 and (b[i] - a[i]) @ (b[i] - a[i]) > 0]
    R, delta = r.uniform(0.03, 0.08), sign * r.uniform(0.01, 0.04)
    k, c = r.uniform(5e3, 5e4), r.uniform(50, 500)
    if what == TWO:
        both = [i for i in live if i + 1 in live]
        i = both[r.randint(len(both))]
        x, u = b[i], _unit(r)
        rad = min(ref.radius[i], ref.radius[i + 1])
    else:
        i = live[r.randint(len(live))]
        rad = ref.radius[i]
        vl = b[i] - a[i]
        ax = vl / np.linalg.norm(vl)
        u = _unit(r)
        if what == T0:
            x, u = a[i], (u if u @ ax < 0 else -u)
        elif what == T1:
            x, u = b[i], (u if u @ ax > 0 else -u)
        else:
            x = a[i] + r.uniform(0.1, 0.9) * vl
            if leave is not None:
                v = ref.jx(i, leave[0], x) @ leave[1]
                u = 0.5 * u - v / max(np.linalg.norm(v), 1e-12)
            u = u - (u @ ax) * ax
            u /= np.linalg.norm(u)
            if leave is not None:
                vn = -u @ v
                push_max = 500.0 * vn / (1 + MARGIN)  # k delta <= c vn / (1 + MARGIN) with c <= 500
                if push_max <= 5e3 * 0.01:
                    return None
                delta = r.uniform(0.01, min(0.04, push_max / 5e3))
                k = r.uniform(5e3, min(5e4, push_max / delta))
                c = r.uniform(max(50.0, (1 + MARGIN) * k * delta / vn), 500)
    return np.array([*(x + u * (R + rad - delta)), R, k, c, r.uniform(0, 1)])


def _row_ok(ref, q, dq, obs, a, b, kind):
    ps = ref.pairs(q, dq, obs, a, b)
    deltas = np.array([p["delta"] for p in ps])
    if np.abs(deltas).min() < GAP or (len(ps) > 1 and np.sort(deltas)[-1] - np.sort(deltas)[-2] < GAP):
        return False
    if min(p["margin"] for p in ps) < MARGIN:
        return False
    pen = [p for p in ps if p["delta"] > 0]
    force = [p for p in pen if p["fn"] > 0]
    first = [p for p in force if p["ob"] == 0]
    if kind == CLEAR:
        return not pen
    if kind == LEAVE:
        return bool(pen) and not force
    if kind == IN:
        return any(0 < p["t"] < 1 for p in first)
    if kind == T0:
        return any(p["t"] == 0 for p in first)
    if kind == T1:
        return any(p["t"] == 1 for p in first)
    segs = sorted(p["seg"] for p in pen if p["ob"] == 0)
    return bool(first) and any(s + 1 in segs for s in segs)


def draw_obstacles(seed, ref, q, dq, K, dtype):
    """-> obstacle [B,K,7] (rounded to dtype, float64), kind [B]"""
    r = np.random.RandomState(seed)
    B = q.shape[0]
    kind = np.arange(B) % 6
    out = np.zeros((B, K, 7))
    for row in range(B):
        a, b = ref.segments(q[row])
        live = [i for i in range(ref.n) if ref.radius[i] >= 0 and (b[i] - a[i]) @ (b[i] - a[i]) > 0]
        if kind[row] == TWO and not any(i + 1 in live for i in live):
            kind[row] = IN
        for attempt in range(4000):
            if kind[row] == LEAVE and attempt == 1000:
                kind[row] = CLEAR  # too slow to leave inside the ranges
            k0 = kind[row]
            obs = [_place(r, ref, a, b, IN if k0 in (CLEAR, LEAVE) else k0, -1 if k0 == CLEAR else 1,
                          (q[row], dq[row]) if k0 == LEAVE else None)]
            if obs[0] is None:
                continue
            for _ in range(1, K):
                push = k0 in PUSHING and r.randint(2)
                obs.append(_place(r, ref, a, b, IN, 1 if push else -1))
            obs = rounded(dtype, np.array(obs))[0]
            if _row_ok(ref, q[row], dq[row], obs, a, b, k0):
                out[row] = obs
                break
        else:
            raise AssertionError(f"row {row}: no draw of kind {kind[row]} holds its margins")
    return out, kind


_cases = {}


def draw_case(table, name, K, B, dtype, seed, off=()):
    """-> dict(q, dq, obstacle (rounded to dtype, float64), radius, ref, tau, report, keep [B], kind [B], pushing [B]).
    `off`: segments to switch off.  Computed once per key and shared: do not write into it.  Asserts the populations
    and the cap on the reference."""
    key = (name, K, B, np.dtype(dtype).name, seed, tuple(off))
    if key in _cases:
        return _cases[key]
    n = int(table["n_joints"])
    dt_ = np.dtype(dtype)
    q, dq = draw(seed, B, n)[:2]
    q, dq = rounded(dtype, q, dq)
    radius = rounded(dtype, np.random.RandomState(seed + 2000).uniform(0.02, 0.05, n))[0]
    radius[list(off)] = -1.0
    ref = LinkContactRef(table, radius)
    obstacle, kind = draw_obstacles(seed + 1000, ref, q, dq, K, dtype)
    tau, rep, margin, gap = ref.step(q, dq, obstacle)
    keep = (margin >= BAND[dt_]) & (gap >= DEPTH_BAND[dt_])
    assert (~keep).sum() <= CAP[dt_], (key, int((~keep).sum()))
    # the branches, read off the reference alone
    force = np.abs(rep[:, :3]).max(axis=1) > 0
    clear, leaving = rep[:, 4] == 0, (rep[:, 4] > 0) & ~force
    assert np.array_equal(force, np.isin(kind, PUSHING)) and np.array_equal(clear, kind == CLEAR)
    if B >= 30:
        pops = [force & (kind == k) for k in (IN, T0, T1)] + [clear, leaving]
        if (kind == TWO).any():
            pops.append(kind == TWO)
        for pop in pops:
            assert pop.sum() >= B / 12, (key, [int(p.sum()) for p in pops])
    _cases[key] = dict(q=q, dq=dq, obstacle=obstacle, radius=radius, ref=ref, tau=tau, report=rep, keep=keep,
                       kind=kind, pushing=force)
    return _cases[key]


def tau_err(tau, want, force):
    """worst row of max|d| / max|ref| over rows [R,n].  A force at the origin of joint 0 (t = 0 on the first segment) has
    no lever: the reference's torque is the rounding of its own kinematics (below 1e-12 m of lever) and the code under
    test must stay below that too - such a row adds nothing to the ratio."""
    lever = 1e-12 * np.abs(force).max(axis=1)
    none = np.abs(want).max(axis=1) <= lever
    assert (np.abs(tau[none]).max(axis=1) <= lever[none]).all() if none.any() else True
    return rel_err(tau[~none], want[~none]) if (~none).any() else 0.0


def check(case, tau, report, dtype, what=""):
    """tau and report of the code under test against the case's reference -> the worst error found (asserted <= bar)"""
    tol = tol_of(dtype)
    f64 = np.dtype(dtype) == np.float64
    on = case["pushing"] & case["keep"]
    off = ~case["pushing"]
    assert np.isfinite(tau).all() and np.isfinite(report).all()
    assert not tau[off].any(), f"{what}: a row without force has tau != 0"
    assert not report[off, :3].any(), f"{what}: a row without force reports one"
    worst = 0.0
    if on.any():
        e_tau = tau_err(tau[on], case["tau"][on], case["report"][on, :3])
        e_f = rel_err(report[on, 0:3], case["report"][on, 0:3])
        print(f"{what}: tau {e_tau:.2e} force {e_f:.2e} (left out {int((~case['keep']).sum())})")
        assert e_tau <= tol and e_f <= tol, (what, e_tau, e_f)
        worst = max(e_tau, e_f)
    # depth and t to the fp32 / fp64 kinematics (absolute: a few 1e-7 m at a 1 m reach in fp32); the integers exactly
    keep = case["keep"]
    dd = np.abs(report[:, 3] - case["report"][:, 3]).max()
    assert dd <= (1e-12 if f64 else 2e-6), (what, dd)
    assert np.array_equal(report[keep, 4:7], case["report"][keep, 4:7]), what
    dt = np.abs(report[keep, 7] - case["report"][keep, 7]).max()
    assert dt <= (1e-10 if f64 else 1e-4), (what, dt)
    return worst
