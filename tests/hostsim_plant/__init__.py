"""Python side of the hostsim_plant TEST AID (tests/hostsim_plant/hostsim_plant.cpp): the plant's two row programs, the
plain one and the one with non-ideal effects, built for the host side by side, one small library per arm table
(compile-time tables) or per joint count (runtime tables).  plain_only=True: a build of its own that holds the plain row
program alone.  Never imported by the product."""
import ctypes as C
import os

import numpy as np

from abr_control_amd import _abi
from tests import hostsim_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_BUILD = os.path.join(_HERE, "build")
_DEPS = hostsim_build.csrc("abrk_device.h", "abrk_ctrl.h", "abrk_rows.h", "abrk_kernels.h", "abrk_rt.h",
                           "abrk_arms_builtin.h", "abrk_sincos_table.h", "abrk_params.h") + [hostsim_build.ABRK_H]
_libs = {}


def _build(key, defs, plain_only):
    if plain_only:
        key, defs = key + "_plain", defs + ["-DHOSTSIM_PLANT_PLAIN_ONLY"]
    if key not in _libs:
        L = C.CDLL(hostsim_build.build(os.path.join(_HERE, "hostsim_plant.cpp"),
                                       os.path.join(_BUILD, f"libhostsim_plant_{key}.so"), _DEPS, defs))
        L.hostsim_plant.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                    C.POINTER(_abi.PlantEffects), C.c_int64] + [C.c_void_p] * 6
        _libs[key] = L
    return _libs[key]


def lib_static(table, plain_only=False):
    """the rows on `table` as a compile-time table (built-in arms, compiled plugins, general-inertia arms)"""
    key, hdr = hostsim_build.table_header(_BUILD, table, "Tab_hostsim_plant")
    return _build(key, ["-include", hdr, "-DHOSTSIM_PLANT_TAB=abrk::Tab_hostsim_plant"], plain_only)


def lib_runtime(n, plain_only=False):
    return _build(f"rt{n}", [f"-DHOSTSIM_PLANT_RT_N={n}"], plain_only)


def _run(table, runtime, plain, plain_only, mode, dt, substeps, gravity, q, dq, u, effects, tau_ext, wrench, dtype):
    dt_ = np.dtype(dtype)
    q = np.array(q, dtype=dt_, order="C")
    dq = np.array(dq, dtype=dt_, order="C")
    u = np.ascontiguousarray(u, dtype=dt_)
    ext = None if tau_ext is None else np.ascontiguousarray(tau_ext, dtype=dt_)
    w = None if wrench is None else np.ascontiguousarray(wrench, dtype=dt_)
    assert ext is None or ext.shape == q.shape
    assert w is None or w.shape == (q.shape[0], 6)
    assert not plain_only or (effects is None and ext is None and w is None)
    ddq = np.full(q.shape, np.nan, dt_)
    if runtime:
        L, desc = lib_runtime(int(table["n_joints"]), plain_only), _abi.desc_from_table(table)
        dp = C.cast(C.byref(desc), C.c_void_p)
    else:
        L, dp = lib_static(table, plain_only), None
    assert L.hostsim_plant_n() == q.shape[1]
    rc = L.hostsim_plant(dp, 0 if dt_ == np.float64 else 1, int(plain or plain_only), mode, float(dt), int(substeps),
                         int(bool(gravity)), None if effects is None else C.byref(effects), q.shape[0], q.ctypes.data,
                         dq.ctypes.data, u.ctypes.data, None if ext is None else ext.ctypes.data,
                         None if w is None else w.ctypes.data, ddq.ctypes.data)
    assert rc in (0, 1), rc
    return q, dq, ddq, rc == 1


def forward_dynamics(table, q, dq, u, effects=None, tau_ext=None, wrench=None, dtype=np.float64, runtime=False,
                     gravity=True, plain=False, plain_only=False):
    """-> ddq [B, n].  plain: the plain row program of the side-by-side build (effects, tau_ext and wrench ignored);
    plain_only: the plain row program of the build that holds nothing else"""
    return _run(table, runtime, plain, plain_only, 0, 1.0, 1, gravity, q, dq, u, effects, tau_ext, wrench, dtype)[2]


def is_singular(table, q, dq, u, dtype=np.float64, runtime=False, plain=False, plain_only=False):
    """did a row's M meet a Cholesky pivot <= 0 (what the kernels report as ABRK_ESINGULAR)?"""
    return _run(table, runtime, plain, plain_only, 0, 1.0, 1, True, q, dq, u, None, None, None, dtype)[3]


def plant_step(table, dt, substeps, q, dq, u, effects=None, tau_ext=None, wrench=None, dtype=np.float64,
               runtime=False, gravity=True, plain=False, plain_only=False):
    """-> (q, dq) after one step of dt (copies; the inputs are left alone)"""
    return _run(table, runtime, plain, plain_only, 1, dt, substeps, gravity, q, dq, u, effects, tau_ext, wrench,
                dtype)[:2]
