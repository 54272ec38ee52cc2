"""Python side of the hostsim_path TEST AID (tests/hostsim_path/hostsim_path.cpp): the path planner's row programs
built for the host on first use.  Never imported by the product."""
import ctypes as C
import os

import numpy as np

from abr_control_amd import _abi
from abr_control_amd.controllers.path_planners.path_planner import profile_tables
from tests import hostsim_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = hostsim_build.build(os.path.join(_HERE, "hostsim_path.cpp"),
                             os.path.join(_HERE, "build", "libhostsim_path.so"), hostsim_build.csrc("abrk_path.h"))
    L = C.CDLL(so)
    head = [C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
    L.hostsim_path_plan.argtypes = head + [C.c_void_p] * 5
    L.hostsim_path_fill.argtypes = head + [C.c_int] + [C.c_void_p] * 8
    _lib = L
    return L


def generate_path(pos_profile, vel_profile, start, target, max_velocity, start_orientation=None,
                  target_orientation=None, start_velocity=0, target_velocity=0, axes="rxyz"):
    """PathPlanner.generate_path for B rows on the host -> (path [B, Tmax, 6 | 12], n_timesteps [B]); n_timesteps is 0
    (and the row zeros) where the row has no path"""
    return fill(pos_profile, vel_profile, start, target, start_orientation, target_orientation, None, 0.0, max_velocity,
                start_velocity, target_velocity, axes, with_counts=True)


def fill(pos_profile, vel_profile, start, target, start_orientation, target_orientation, t_max, sentinel, max_velocity,
         start_velocity=0, target_velocity=0, axes="rxyz", with_counts=False):
    """the plan pass, then the fill and gradient passes into a [B, t_max, 6 | 12] array that held `sentinel` everywhere
    (t_max None: the largest step count) -> path, or (path, n_timesteps)"""
    f8 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    start, target, so, to = f8(start), f8(target), f8(start_orientation), f8(target_orientation)
    B, W = start.shape[0], 6 if so is None else 12
    table, off, cands = profile_tables(pos_profile, vel_profile, max_velocity, start_velocity, target_velocity)
    S, K = int(pos_profile.n_sample_points), len(cands)
    nt, rowplan, ds = np.zeros(B, np.int32), np.zeros((B, 2), np.int32), np.zeros((B, S))
    p = lambda a: None if a is None else a.ctypes.data
    head = (float(vel_profile.dt), S, K, _abi.euler_axes_code(axes), W, p(table), p(off), B)
    L = lib()
    L.hostsim_path_plan(*head, p(start), p(target), p(nt), p(rowplan), p(ds))
    if t_max is None:
        t_max = max(int(nt.max()), 1)
    path = np.full((B, t_max, W), float(sentinel))
    L.hostsim_path_fill(*head, t_max, p(start), p(target), p(so), p(to), p(nt), p(rowplan), p(ds), p(path))
    return (path, nt) if with_counts else path
