"""Python side of the hostsim_gi TEST AID (tests/hostsim_gi/hostsim_gi.cpp): the row programs built for the host on a
general-inertia arm table, one small library per table.  Never imported by the product."""
import ctypes as C
import os

import numpy as np

from abr_control_amd.engine import _OUT_SHAPES, _WANT_BITS
from tests import hostsim_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_BUILD = os.path.join(_HERE, "build")
_DEPS = hostsim_build.csrc("abrk_device.h", "abrk_ctrl.h", "abrk_rows.h", "abrk_arms_builtin.h", "abrk_sincos_table.h")
_libs = {}


def lib_for(table):
    """the host build of the row programs on `table` (built on first use, rebuilt when a source is newer)"""
    key, hdr = hostsim_build.table_header(_BUILD, table, "Tab_hostsim_gi")
    if key not in _libs:
        _libs[key] = C.CDLL(hostsim_build.build(
            os.path.join(_HERE, "hostsim_gi.cpp"), os.path.join(_BUILD, f"libhostsim_gi_{key}.so"), _DEPS,
            ["-include", hdr, "-DHOSTSIM_GI_TAB=abrk::Tab_hostsim_gi"]))
    return _libs[key]


def _code(dt):
    return 0 if np.dtype(dt) == np.float64 else 1


def dynamics(table, q, dq=None, frame=None, want=("M", "g"), dtype=np.float64):
    L = lib_for(table)
    n = L.hostsim_gi_n()
    dt = np.dtype(dtype)
    q = np.ascontiguousarray(q, dtype=dt)
    dq = None if dq is None else np.ascontiguousarray(dq, dtype=dt)
    B = q.shape[0]
    frame = 2 * n + 1 if frame is None else frame
    outs = (C.c_void_p * 10)()
    names = ("Tx", "J", "M", "g", "C", "dJ", "R", "T", "Tinv", "quat")
    res, bits = {}, 0
    for w in want:
        bits |= _WANT_BITS[w]
        res[w] = np.full((B,) + _OUT_SHAPES[w](n), np.nan, dt)
        outs[names.index(w)] = res[w].ctypes.data
    rc = L.hostsim_gi_dynamics(_code(dt), C.c_int64(B), C.c_void_p(q.ctypes.data),
                               None if dq is None else C.c_void_p(dq.ctypes.data), frame, C.c_uint32(bits), outs)
    assert rc == 0, rc
    return res


def coriolis_vector(table, q, dq, dtype=np.float64):
    """C(q, dq) dq as the OSC kernels of general-inertia arms accumulate it"""
    L = lib_for(table)
    dt = np.dtype(dtype)
    q, dq = np.ascontiguousarray(q, dtype=dt), np.ascontiguousarray(dq, dtype=dt)
    out = np.full(q.shape, np.nan, dt)
    rc = L.hostsim_gi_cvec(_code(dt), C.c_int64(q.shape[0]), C.c_void_p(q.ctypes.data), C.c_void_p(dq.ctypes.data),
                           C.c_void_p(out.ctypes.data))
    assert rc == 0, rc
    return out
