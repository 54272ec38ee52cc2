"""Path planners on the batched engine.

InverseKinematics (abr_control/controllers/path_planners/inverse_kinematics.py:28-135): all iterations of a path in one
kernel.  PathPlanner (path_planner.py:13-475) with its position profiles, velocity profiles and the Orientation
planner: one movement or a batch of B movements per generate_path call - the profile objects are sampled once per call
on the host, every row's path is planned and filled in on the device, and `engine.path_next` feeds a recorded control
loop from the device-resident result (DESIGN.md "Path planner")."""
from . import position_profiles, velocity_profiles
from .inverse_kinematics import InverseKinematics
from .orientation import Orientation
from .path_planner import PathPlanner
from .position_profiles import Ellipse, FromPoints, PosProf, SinCurve
from .velocity_profiles import Gaussian, VelProf

__all__ = ["InverseKinematics", "PathPlanner", "Orientation", "position_profiles", "velocity_profiles", "PosProf",
           "SinCurve", "FromPoints", "Ellipse", "VelProf", "Gaussian"]
