#!/usr/bin/env python3
"""Fixtures of the general-inertia arms (tests/golden/inertia_<arm>.{json,npz}) by RUNNING THE REFERENCE ITSELF.

TEST INFRASTRUCTURE - not part of the product.  Runs where the reference is importable (a scratch copy of it is made
by oracle/gen_golden.py's make_scratch, as for the other fixtures); the GPU box only ever sees the committed files.

For each arm it
  * writes the arm table with full link inertias (`mlink`) and joint inertias (`mjoint`),
  * builds a reference `BaseConfig` subclass from that table: the symbolic chain
        T(link0) = A0,  T(joint_i) = T(link_i) AJ[i],  T(link_i+1) = T(joint_i) Rz(q_i) B[i],  T(EE) = T(link_n) E
    with `J_orientation[i] = T(joint_i)[:3, :3] z` as the shipped configs set it, and `_M_LINKS` / `_M_JOINTS` from the
    table,
  * stores the reference's SymPy M, g (and C where affordable), J of every frame and dJ, evaluated in fp64 without the
    float32 cast of the public wrappers (Oracle-D), at seeded (q, dq),
  * and the outputs of the reference's own OSC, Sliding, Joint and Floating on that config (Oracle-D as well).

Arms:  synthetic4 - tests/synthetic_arms.make_arm(4, 204, True) with random symmetric positive definite link inertias
                    (non-zero linear-angular blocks) and non-zero joint inertias on every joint, joint 0 included;
       ur5        - the UR5 table with rotor inertias on the angular diagonal of every joint (M, g and the
                    controllers that do not need C: SymPy's C of a six-joint arm takes too long here).

Usage:  python tools/gen_inertia_golden.py [synthetic4] [ur5]
"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
B_DYN = 12  # states of the dynamics arrays
B_CTRL = 12  # states per controller case


def spatial_inertia(rng, m, spread):
    """6x6 inertia of a body whose centre of mass sits `spread` away from the frame origin, with a rotated principal
    frame: symmetric positive definite, non-diagonal angular block, non-zero linear-angular blocks"""
    c = rng.uniform(-spread, spread, 3)
    cx = np.array([[0, -c[2], c[1]], [c[2], 0, -c[0]], [-c[1], c[0], 0]])
    a = rng.normal(size=(3, 3))
    Q, _ = np.linalg.qr(a)
    Ic = Q @ np.diag(rng.uniform(0.01, 0.08, 3)) @ Q.T
    out = np.zeros((6, 6))
    out[:3, :3] = m * np.eye(3)
    out[:3, 3:] = -m * cx
    out[3:, :3] = m * cx
    out[3:, 3:] = Ic - m * cx @ cx
    return np.round(0.5 * (out + out.T), 12)


def make_tables():
    sys.path.insert(0, REPO)
    from abr_control_amd import _abi
    from tests.synthetic_arms import make_arm

    rng = np.random.RandomState(4204)
    s4 = make_arm(4, 204, True)
    s4["name"] = "synthetic4_gi"
    ml = [np.zeros((6, 6))]
    for l in range(1, 5):
        ml.append(spatial_inertia(rng, s4["mdiag"][l][0], 0.08))
    mj = [spatial_inertia(rng, rng.uniform(0.05, 0.3), 0.03) for _ in range(4)]
    s4["mdiag"] = [np.diag(m).tolist() for m in ml]
    s4["mlink"] = [m.tolist() for m in ml]
    s4["mjoint"] = [m.tolist() for m in mj]

    ur5 = dict(_abi.load_table("ur5"))
    ur5["name"] = "ur5_rotors"
    rot = [0.012, 0.015, 0.010, 0.004, 0.004, 0.003]
    ur5["mjoint"] = [np.diag([0, 0, 0, 0.3 * r, 0.5 * r, r]).tolist() for r in rot]
    return {"synthetic4": s4, "ur5": ur5}


# ---------------------------------------------------------------------------- worker (reference importable)
def worker(arm, table_path, out_path):
    import sympy as sp
    from abr_control.arms.base_config import BaseConfig
    from abr_control.controllers import OSC, Floating, Joint, Sliding

    tab = json.load(open(table_path))
    n = int(tab["n_joints"])

    class TableConfig(BaseConfig):
        def __init__(self, **kw):
            super().__init__(N_JOINTS=n, N_LINKS=int(tab["n_links_dyn"]), ROBOT_NAME=f"abrk_gi_{tab['name']}", **kw)
            aff = lambda m: sp.Matrix(np.vstack([np.asarray(m, float), [0, 0, 0, 1]]).tolist())
            self.A0 = aff(tab["A0"])
            self.AJ = [aff(m) for m in tab["AJ"]]
            self.B = [aff(m) for m in tab["B"]]
            self.E = aff(tab["E"])
            self._T = {}
            self._M_LINKS = [sp.Matrix(np.asarray(m, float).tolist()) for m in tab["mlink"]] if "mlink" in tab else [
                sp.diag(*[float(v) for v in r]) for r in tab["mdiag"]]
            self._M_JOINTS = [sp.Matrix(np.asarray(m, float).tolist()) for m in tab["mjoint"]]
            self.J_orientation = [self._calc_T(f"joint{i}")[:3, :3] * self._KZ for i in range(n)]

        def _calc_T(self, name):
            if self._T.get(name) is None:
                if name == "link0":
                    T = self.A0
                elif name == "EE":
                    T = self._calc_T(f"link{n}") * self.E
                elif name.startswith("joint"):
                    i = int(name[5:])
                    T = self._calc_T(f"link{i}") * self.AJ[i]
                elif name.startswith("link"):
                    i = int(name[4:]) - 1
                    c, s = sp.cos(self.q[i]), sp.sin(self.q[i])
                    Rz = sp.Matrix([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
                    T = self._calc_T(f"joint{i}") * Rz * self.B[i]
                else:
                    raise Exception(f"Invalid transformation name: {name}")
                self._T[name] = T
            return self._T[name]

    rc = TableConfig(use_cython=False)

    class Raw:
        """Oracle-D: the reference's generated functions without the float32 cast of its wrappers"""

        def __init__(self, rc):
            self.rc, self.N_JOINTS, self.N_LINKS, self.x_zeros = rc, rc.N_JOINTS, rc.N_LINKS, np.zeros(3)

        def _fn(self, name, x):
            x = self.x_zeros if x is None else x
            return x, (name + "[0,0,0]" if np.allclose(x, 0) else name)

        def g(self, q):
            self.rc.g(q)
            return np.array(self.rc._g(*tuple(q)), dtype="float64").flatten()

        def M(self, q):
            self.rc.M(q)
            return np.array(self.rc._M(*tuple(q)), dtype="float64")

        def C(self, q, dq):
            self.rc.C(q, dq)
            return np.array(self.rc._C(*(tuple(q) + tuple(dq))), dtype="float64")

        def J(self, name, q, x=None):
            self.rc.J(name, q, x)
            x, fn = self._fn(name, x)
            return np.array(self.rc._J[fn](*(tuple(q) + tuple(x))), dtype="float64")

        def dJ(self, name, q, dq, x=None):
            self.rc.dJ(name, q, dq, x)
            x, fn = self._fn(name, x)
            return np.array(self.rc._dJ[fn](*(tuple(q) + tuple(dq) + tuple(x))), dtype="float64")

        def R(self, name, q):
            self.rc.R(name, q)
            return np.array(self.rc._R[name](*tuple(q)), dtype="float64")

        def quaternion(self, name, q):
            from abr_control.utils import transformations

            return transformations.unit_vector(transformations.quaternion_from_matrix(matrix=self.R(name, q)))

        def Tx(self, name, q, x=None):
            return self.rc.Tx(name, q, x)

    raw = Raw(rc)
    with_C = arm != "ur5"
    out = {}
    rng = np.random.RandomState(7)
    q = rng.uniform(0, 2 * np.pi, (B_DYN, n))
    dq = rng.uniform(-3, 3, (B_DYN, n))
    out["dyn_q"], out["dyn_dq"] = q, dq
    frames = [f for i in range(n + 1) for f in ((f"link{i}", f"joint{i}") if i < n else (f"link{i}",))] + ["EE"]
    out["frames"] = np.array(frames)
    out["M"] = np.array([raw.M(x) for x in q])
    out["g"] = np.array([raw.g(x) for x in q])
    print(f"  {arm}: M, g done", flush=True)
    for f in frames:
        out[f"J_{f}"] = np.array([raw.J(f, x) for x in q])
    if with_C:
        out["C"] = np.array([raw.C(a, b) for a, b in zip(q, dq)])
        for f in frames:
            out[f"dJ_{f}"] = np.array([raw.dJ(f, a, b) for a, b in zip(q, dq)])
        print(f"  {arm}: C, dJ done", flush=True)

    def states(seed, nt):
        r = np.random.RandomState(seed)
        return r.uniform(0, 2 * np.pi, (B_CTRL, n)), r.uniform(0, 3, (B_CTRL, n)), r.uniform(-1, 1, (B_CTRL, nt))

    def case(key, seed, nt, make, call):
        qq, dd, tt = states(seed, nt)
        out[f"{key}_q"], out[f"{key}_dq"], out[f"{key}_target"] = qq, dd, tt
        out[f"{key}_u"] = np.array([call(make(), qq[b], dd[b], tt[b]) for b in range(B_CTRL)])
        print(f"  {arm}: {key} done", flush=True)

    xyz, six = [True, True, True, False, False, False], [True] * 6
    for use_C in ((False, True) if with_C else (False,)):
        c = "_C" if use_C else ""
        case(f"osc_xyz{c}", 10 + use_C, 6, lambda: OSC(raw, kp=200, ctrlr_dof=xyz, use_C=use_C),
             lambda o, a, b, t: o.generate(a, b, t))
        case(f"osc6{c}", 20 + use_C, 6, lambda: OSC(raw, kp=200, ko=150, kv=25, ctrlr_dof=six, use_C=use_C),
             lambda o, a, b, t: o.generate(a, b, t))
    if with_C:
        case("sliding", 30, 3, lambda: Sliding(raw), lambda o, a, b, t: o.generate(a, b, t))
    case("joint", 31, n, lambda: Joint(raw, kp=50, kv=9), lambda o, a, b, t: o.generate(a, b, t * 3.0))
    case("floating", 32, n, lambda: Floating(raw, dynamic=True), lambda o, a, b, t: o.generate(a, b))
    np.savez_compressed(out_path, **out)
    print(f"  wrote {out_path} ({len(out)} arrays)", flush=True)


def main():
    if sys.argv[1:2] == ["--worker"]:
        return worker(*sys.argv[2:5])
    which = sys.argv[1:] or ["synthetic4", "ur5"]
    tables = make_tables()
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    from gen_golden import make_scratch

    scratch = make_scratch()
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=scratch)
    try:
        for arm in which:
            tp = os.path.join(OUT, f"inertia_{arm}.json")
            with open(tp, "w") as fh:
                json.dump(tables[arm], fh, indent=1)
                fh.write("\n")
            print(f"==== {arm}", flush=True)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", arm, tp,
                            os.path.join(OUT, f"inertia_{arm}.npz")], env=env, check=True)
    finally:
        shutil.rmtree(os.path.dirname(scratch), ignore_errors=True)


if __name__ == "__main__":
    main()
