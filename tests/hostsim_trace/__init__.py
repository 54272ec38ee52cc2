"""Python side of the hostsim_trace TEST AID (tests/hostsim_trace/hostsim_trace.cpp): the loop recorder's row program
built for the host, one small library per arm table (compile-time tables) or per joint count (runtime tables).  Never
imported by the product."""
import ctypes as C
import os

import numpy as np

from abr_control_amd import _abi
from tests import hostsim_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_BUILD = os.path.join(_HERE, "build")
_DEPS = hostsim_build.csrc("abrk_device.h", "abrk_ctrl.h", "abrk_rows.h", "abrk_trace.h", "abrk_rt.h",
                           "abrk_arms_builtin.h", "abrk_sincos_table.h")
_libs = {}


def _build(key, defs):
    if key not in _libs:
        L = C.CDLL(hostsim_build.build(os.path.join(_HERE, "hostsim_trace.cpp"),
                                       os.path.join(_BUILD, f"libhostsim_trace_{key}.so"), _DEPS, defs))
        L.hostsim_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_uint,
                                    C.c_double, C.c_int64] + [C.c_void_p] * 8
        _libs[key] = L
    return _libs[key]


def lib_static(table):
    """the row on `table` as a compile-time table (built-in arms, compiled plugins)"""
    key, hdr = hostsim_build.table_header(_BUILD, table, "Tab_hostsim_trace")
    return _build(key, ["-include", hdr, "-DHOSTSIM_TRACE_TAB=abrk::Tab_hostsim_trace"])


def lib_runtime(n):
    return _build(f"rt{n}", [f"-DHOSTSIM_TRACE_RT_N={n}"])


class HostTrace:
    """engine.loop_trace on the host: the same arguments (NumPy arrays, updated in place), one tick per call"""

    def __init__(self, table, runtime=False):
        self.n = int(table["n_joints"])
        if runtime:
            self.L, self._desc = lib_runtime(self.n), _abi.desc_from_table(table)
            self.dp = C.cast(C.byref(self._desc), C.c_void_p)
        else:
            self.L, self.dp = lib_static(table), None
        assert self.L.hostsim_trace_n() == self.n

    def __call__(self, params, q, dq, u, target, counter, history=None, stats=None, settle=None, dtype=np.float64):
        dt = np.dtype(dtype)
        ins = [None if x is None else np.ascontiguousarray(x, dtype=dt) for x in (q, dq, u, target)]
        for arr, t in ((counter, np.int32), (history, dt), (stats, np.float64), (settle, np.int32)):
            assert arr is None or (arr.dtype == t and arr.flags.c_contiguous)
        p = [None if x is None else x.ctypes.data for x in ins + [counter, history, stats, settle]]
        rc = self.L.hostsim_trace(self.dp, 0 if dt == np.float64 else 1, params.frame, params.x_off, params.every,
                                  params.capacity, params.columns if history is not None else 0, params.tol,
                                  counter.shape[0], *p)
        assert rc == 0, rc
