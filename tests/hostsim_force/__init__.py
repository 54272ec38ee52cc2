"""Python side of the hostsim_force TEST AID (tests/hostsim_force/hostsim_force.cpp): the row program of the force-control
law (force_body) built for the host, one small library per arm table (compile-time tables) or per joint count (runtime
tables).  Never imported by the product."""
import ctypes as C
import os

import numpy as np

from abr_control_amd import _abi
from tests import hostsim_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_BUILD = os.path.join(_HERE, "build")
_DEPS = hostsim_build.csrc("abrk_device.h", "abrk_ctrl.h", "abrk_rows.h", "abrk_force.h", "abrk_rt.h",
                           "abrk_arms_builtin.h", "abrk_sincos_table.h") + [hostsim_build.ABRK_H]
_libs = {}


def _build(key, defs):
    if key not in _libs:
        L = C.CDLL(hostsim_build.build(os.path.join(_HERE, "hostsim_force.cpp"),
                                       os.path.join(_BUILD, f"libhostsim_force_{key}.so"), _DEPS, defs))
        L.hostsim_force.argtypes = [C.c_void_p, C.c_int, C.POINTER(_abi.ForceParams), C.c_int64] + [C.c_void_p] * 8 + [
            C.POINTER(C.c_int)]
        _libs[key] = L
    return _libs[key]


def lib_static(table):
    """the row on `table` as a compile-time table (built-in arms, compiled plugins)"""
    key, hdr = hostsim_build.table_header(_BUILD, table, "Tab_hostsim_force")
    return _build(key, ["-include", hdr, "-DHOSTSIM_FORCE_TAB=abrk::Tab_hostsim_force"])


def lib_runtime(n):
    return _build(f"rt{n}", [f"-DHOSTSIM_FORCE_RT_N={n}"])


def force_step(table, params, q, dq, target, cmd, force, integ, target_velocity=None, u=None, dtype=np.float64,
               runtime=False):
    """-> (u [B, n], integ [B], singular) of `dtype`.  params: _abi.ForceParams (force_ld = the columns of `force`);
    integ: the integral before the tick (a copy is advanced); u: an array to ADD to with params.accumulate (a copy is
    made), else None"""
    dt_ = np.dtype(dtype)
    n = int(table["n_joints"])
    arr = lambda x: np.ascontiguousarray(x, dtype=dt_)  # noqa: E731
    q, dq, target, cmd, force = arr(q), arr(dq), arr(target), arr(cmd), arr(force)
    B = q.shape[0]
    assert q.shape == (B, n) and dq.shape == (B, n) and target.shape == (B, 6) and cmd.shape == (B, 4)
    assert force.shape == (B, params.force_ld)
    tv = None if target_velocity is None else arr(target_velocity)
    assert tv is None or tv.shape == (B, 6)
    assert bool(params.accumulate) == (u is not None)
    out = np.array(u, dtype=dt_, order="C") if u is not None else np.full((B, n), np.nan, dt_)
    state = np.array(integ, dtype=dt_, order="C")
    assert state.shape == (B,)
    if runtime:
        L, desc = lib_runtime(n), _abi.desc_from_table(table)
        dp = C.cast(C.byref(desc), C.c_void_p)
    else:
        L, dp = lib_static(table), None
    assert L.hostsim_force_n() == n
    status = C.c_int(0)
    rc = L.hostsim_force(dp, 0 if dt_ == np.float64 else 1, C.byref(params), B, q.ctypes.data, dq.ctypes.data,
                         target.ctypes.data, None if tv is None else tv.ctypes.data, cmd.ctypes.data,
                         force.ctypes.data, state.ctypes.data, out.ctypes.data, C.byref(status))
    assert rc == 0, rc
    return out, state, bool(status.value)
