"""Reference of the plant with a payload at the end effector (include/abrk.h, abrk_plant_step_payload_batch), restated in
NumPy on the oracle: the reference of the effects tests (tests/plant_fx_ref.py RefFx) with step 3 replaced by
  Jp = J("EE", q, x=r)[:3];  dJp = dJ("EE", q, dq, x=r)[:3]
  ddq = solve(M + m Jp^T Jp, tau - C dq - m Jp^T (dJp dq) - g - Jp^T m (0, 0, -9.81))
for a point mass m at offset r (EE frame) per row; gravity off leaves both gravity terms out.  General-inertia arms take
M, C, g from the host build of the dynamics row program (HostsimGiDyn), their kinematics are the oracle's.  Shared by the
CPU and the GPU tests; fed inputs already rounded to the dtype under test (rounded())."""
import numpy as np

from tests.plant_fx_ref import ALL_ON, BAND, CAP, TOL_F32, TOL_F64, HostsimGiDyn, OracleDyn, RefFx, draw, \
    effects_rounded, effects_struct, gi_table, rel_err, rounded  # noqa: F401  (re-exported to the tests)

SEED, SEED_PAYLOAD = 41, 43
GRAV = np.array([0.0, 0.0, -9.81])


def draw_payload(seed, B):
    """-> [B, 4] of m, rx, ry, rz: m in 0.2 - 3 kg, r within 10 cm; every seventh row carries nothing"""
    r = np.random.RandomState(seed)
    m = r.uniform(0.2, 3.0, B)
    off = r.uniform(-0.1, 0.1, (B, 3))
    m[::7] = 0
    return np.concatenate([m[:, None], off], axis=1)


class RefPayload(RefFx):
    """RefFx whose rows carry `payload` [B, 4] (replaceable between calls: set_payload)"""

    def __init__(self, dyn, table, payload=None):
        super().__init__(dyn, table)
        self.payload = payload

    def set_payload(self, payload):
        self.payload = None if payload is None else np.asarray(payload, dtype=np.float64)
        return self

    def ddq(self, q, dq, u, fx=None, tau_ext=None, wrench=None, gravity=True):
        if self.payload is None:
            return super().ddq(q, dq, u, fx, tau_ext, wrench, gravity)
        assert self.payload.shape == (q.shape[0], 4)
        out = np.empty_like(q)
        for b in range(q.shape[0]):
            m, r = self.payload[b, 0], self.payload[b, 1:]
            M, Cm, g = self.dyn(q[b], dq[b])
            tau = self.tau(q[b], dq[b], u[b], fx, None if tau_ext is None else tau_ext[b],
                           None if wrench is None else wrench[b])
            Jp = self.O.J("EE", q[b], x=r)[:3]
            dJp = self.O.dJ("EE", q[b], dq[b], x=r)[:3]
            rhs = tau - Cm @ dq[b] - m * Jp.T @ (dJp @ dq[b])
            if gravity:
                rhs = rhs - g - Jp.T @ (m * GRAV)
            out[b] = np.linalg.solve(M + m * Jp.T @ Jp, rhs)
        return out
