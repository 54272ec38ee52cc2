import numpy as np

from .. import _abi, engine
from .._lib import DeviceArray
from ..sharding import ShardedArray

RESIDENT = (DeviceArray, ShardedArray)  # arrays that live on devices: passed through as they are, returned in kind


class Controller:
    """Base of all controllers (abr_control/controllers/controller.py:4-32).

    The controllers that sharding.MultiDevice can run (OSC, Sliding, Joint, Damping, RestingConfig) keep the one body
    of their generate() in `_generate(where, q, dq, ...)`.  where: None - this config's device, what generate() passes;
    a list of device ordinals - the host batch is cut over them; the streams of the shards - q and the other arrays
    are ShardedArrays resident on the devices."""

    def __init__(self, robot_config):
        self.robot_config = robot_config
        self.offset_zeros = np.zeros(3)

    def generate(self, q, dq):
        raise NotImplementedError

    # ---- shared plumbing for the batched device calls
    def _rows(self, *arrays):
        """Normalise (n,) / (B,n) NumPy inputs to 2-D; DeviceArrays and ShardedArrays pass through.
        Returns (arrays, single)"""
        if isinstance(arrays[0], RESIDENT):
            return arrays, False
        dt = self.robot_config.dtype
        single = np.ndim(arrays[0]) == 1
        out = []
        B = np.atleast_2d(np.asarray(arrays[0])).shape[0]
        for a in arrays:
            if a is None:
                out.append(None)
                continue
            a = np.atleast_2d(np.asarray(a, dtype=dt))
            if a.shape[0] == 1 and B > 1:  # one target for the whole batch
                a = np.broadcast_to(a, (B, a.shape[1]))
            out.append(np.ascontiguousarray(a))
        return out, single

    def _marshal(self, where, q2):
        rc = self.robot_config
        if where is None and not isinstance(q2, ShardedArray):  # (shards name their devices themselves)
            where = rc.device
        return engine._marshaller(where, rc.dtype, q2)

    def _joint_generate(self, where, ctrl, account_for_gravity, q, dq, target=None, target_velocity=None):
        """the whole generate() of Joint / Damping / RestingConfig: one kernel"""
        rc = self.robot_config
        (q2, dq2, t2, tv2), single = self._rows(q, dq, target, target_velocity)
        u = engine._joint(self._marshal(where, q2), rc.arm_id, rc.N_JOINTS, ctrl, account_for_gravity, q2, dq2, t2, tv2)
        if isinstance(u, np.ndarray) and rc.reference_dtypes:
            u = u.astype(np.float64)
        return u[0] if single else u

    def _require_batched_config(self):
        from ..arms.base_config import BatchedConfig

        if not isinstance(self.robot_config, BatchedConfig):
            raise TypeError(
                f"{type(self).__name__} of abr_control_amd evaluates on the GPU and needs an "
                "abr_control_amd arm config (abr_control_amd.arms.<arm>.Config or arms.from_table(...)); "
                f"got {type(self.robot_config).__name__}. There is no CPU fallback."
            )


class NullJoint:
    """What Damping and RestingConfig share: they are the Joint kernel without a target, `self._ctrl()` its
    abrk_null_ctrl.  (A mixin, so that `_accumulate` exists on these two classes alone: OSC asks for it.)"""

    def generate(self, q, dq):
        return self._generate(None, q, dq)

    def _generate(self, where, q, dq):
        return self._joint_generate(where, self._ctrl(), False, q, dq)

    def _accumulate(self, q2, dq2, u):
        """u += generate(q2, dq2): used by OSC when more than ABRK_MAX_NULL Damping / RestingConfig controllers are
        given (the first ABRK_MAX_NULL are fused into its kernel; the rest enter through u_null_ext)"""
        if not isinstance(u, np.ndarray):
            raise TypeError(f"more than {_abi.MAX_NULL} fused null controllers need NumPy states")
        rc = self.robot_config
        u += engine.joint_generate(rc.arm_id, rc.N_JOINTS, self._ctrl(), False, q2, dq2, dtype=rc.dtype, device=rc.device)
