"""Adaptive signals with the reference's API (abr_control/controllers/signals/__init__.py), computed on the GPU."""
from .dynamics_adaptation import DynamicsAdaptation

__all__ = ["DynamicsAdaptation"]
