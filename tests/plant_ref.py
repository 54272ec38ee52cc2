"""Reference values of the plant tests: the oracle's M, C, g composed in NumPy (LU solve), and the plain loop of the
reference's update (arms/twojoint/arm_sim.py:131-132).  Shared by the CPU and the GPU plant tests."""
import json
import os

import numpy as np

from oracle.oracle import Oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_F64 = 1e-6   # the project's bars: max|d| / max|ref| per row
TOL_F32 = 1e-4


def draw(seed, B, n):
    """q ~ U(-pi, pi), dq ~ U(-2, 2), u ~ U(-20, 20)"""
    r = np.random.RandomState(seed)
    return r.uniform(-np.pi, np.pi, (B, n)), r.uniform(-2, 2, (B, n)), r.uniform(-20, 20, (B, n))


class OracleDyn:
    def __init__(self, table):
        self.O = Oracle(table)

    def mcg(self, q, dq):
        return self.O.M(q), self.O.C(q, dq), self.O.g(q)


class HostsimGiDyn:
    """M, C, g of a general-inertia table: the host build of the dynamics row program, which tests/test_general_inertia.py
    pins to the reference's fixtures (the oracle library knows diagonal inertias only)"""

    def __init__(self, table):
        self.table = table

    def mcg(self, q, dq):
        from tests import hostsim_gi

        r = hostsim_gi.dynamics(self.table, q[None], dq[None], want=("M", "g", "C"))
        return r["M"][0], r["C"][0], r["g"][0]


def gi_table(name):
    """the general-inertia arm table of tests/golden/inertia_<name>.json, as committed (not normalised)"""
    with open(os.path.join(GOLDEN, f"inertia_{name}.json")) as fh:
        return json.load(fh)


class Ref:
    def __init__(self, dyn):
        self.dyn = dyn.mcg

    def ddq(self, q, dq, u, gravity=True):
        out = np.empty_like(q)
        for b in range(q.shape[0]):
            M, Cm, g = self.dyn(q[b], dq[b])
            out[b] = np.linalg.solve(M, u[b] - Cm @ dq[b] - (g if gravity else 0.0))
        return out

    def steps(self, q, dq, u, dt, substeps=1, n_steps=1, gravity=True):
        q, dq = q.copy(), dq.copy()
        h = dt / substeps
        for _ in range(n_steps * substeps):
            dq += self.ddq(q, dq, u, gravity) * h
            q += dq * h
        return q, dq


def rel_err(got, ref):
    """worst row of max|d| / max|ref| - every row counts"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float(np.max(np.max(np.abs(got - ref), axis=1) / np.max(np.abs(ref), axis=1)))
