"""Null-space damping controller (abr_control/controllers/damping.py:6-32): u = M (-kv dq)."""
from .. import _abi
from .controller import Controller, NullJoint


class Damping(NullJoint, Controller):
    def __init__(self, robot_config, kv):
        super().__init__(robot_config)
        self._require_batched_config()
        self.kv = kv

    def _ctrl(self):
        return _abi.make_damping(self.kv)
