"""Python side of the hostsim_payload TEST AID (tests/hostsim_payload/hostsim_payload.cpp): the row program of the plant
with a payload at the end effector (plant_load_row) built for the host, one small library per arm table (compile-time
tables) or per joint count (runtime tables).  Never imported by the product."""
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


def _build(key, defs):
    if key not in _libs:
        L = C.CDLL(hostsim_build.build(os.path.join(_HERE, "hostsim_payload.cpp"),
                                       os.path.join(_BUILD, f"libhostsim_payload_{key}.so"), _DEPS, defs))
        L.hostsim_payload.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                      C.POINTER(_abi.PlantEffects), C.c_int64] + [C.c_void_p] * 7
        _libs[key] = L
    return _libs[key]


def lib_static(table):
    """the row on `table` as a compile-time table (built-in arms, compiled plugins, general-inertia arms)"""
    key, hdr = hostsim_build.table_header(_BUILD, table, "Tab_hostsim_payload")
    return _build(key, ["-include", hdr, "-DHOSTSIM_PAYLOAD_TAB=abrk::Tab_hostsim_payload"])


def lib_runtime(n):
    return _build(f"rt{n}", [f"-DHOSTSIM_PAYLOAD_RT_N={n}"])


def _run(table, runtime, mode, dt, substeps, gravity, q, dq, u, payload, effects, tau_ext, wrench, dtype):
    dt_ = np.dtype(dtype)
    q = np.array(q, dtype=dt_, order="C")
    dq = np.array(dq, dtype=dt_, order="C")
    u = np.ascontiguousarray(u, dtype=dt_)
    p = np.ascontiguousarray(payload, dtype=dt_)
    ext = None if tau_ext is None else np.ascontiguousarray(tau_ext, dtype=dt_)
    w = None if wrench is None else np.ascontiguousarray(wrench, dtype=dt_)
    assert p.shape == (q.shape[0], 4)
    assert ext is None or ext.shape == q.shape
    assert w is None or w.shape == (q.shape[0], 6)
    ddq = np.full(q.shape, np.nan, dt_)
    if runtime:
        L, desc = lib_runtime(int(table["n_joints"])), _abi.desc_from_table(table)
        dp = C.cast(C.byref(desc), C.c_void_p)
    else:
        L, dp = lib_static(table), None
    assert L.hostsim_payload_n() == q.shape[1]
    rc = L.hostsim_payload(dp, 0 if dt_ == np.float64 else 1, mode, float(dt), int(substeps), int(bool(gravity)),
                           None if effects is None else C.byref(effects), q.shape[0], q.ctypes.data, dq.ctypes.data,
                           u.ctypes.data, None if ext is None else ext.ctypes.data,
                           None if w is None else w.ctypes.data, p.ctypes.data, ddq.ctypes.data)
    assert rc in (0, 1), rc
    return q, dq, ddq, rc == 1


def forward_dynamics(table, q, dq, u, payload, effects=None, tau_ext=None, wrench=None, dtype=np.float64,
                     runtime=False, gravity=True):
    """-> ddq [B, n]"""
    return _run(table, runtime, 0, 1.0, 1, gravity, q, dq, u, payload, effects, tau_ext, wrench, dtype)[2]


def plant_step(table, dt, substeps, q, dq, u, payload, effects=None, tau_ext=None, wrench=None, dtype=np.float64,
               runtime=False, gravity=True):
    """-> (q, dq) after one step of dt (copies; the inputs are left alone)"""
    return _run(table, runtime, 1, dt, substeps, gravity, q, dq, u, payload, effects, tau_ext, wrench, dtype)[:2]
