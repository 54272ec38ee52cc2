"""Python side of the hostsim_contact TEST AID (tests/hostsim_contact/hostsim_contact.cpp): the row program of the
end-effector contact (contact_body) built for the host, one small library per arm table (compile-time tables) or per joint
count (runtime tables).  Never imported by the product."""
import ctypes as C
import os

import numpy as np

from abr_control_amd import _abi
from tests import hostsim_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_BUILD = os.path.join(_HERE, "build")
_DEPS = hostsim_build.csrc("abrk_device.h", "abrk_ctrl.h", "abrk_rows.h", "abrk_contact.h", "abrk_rt.h",
                           "abrk_arms_builtin.h", "abrk_sincos_table.h") + [hostsim_build.ABRK_H]
_libs = {}


def _build(key, defs):
    if key not in _libs:
        L = C.CDLL(hostsim_build.build(os.path.join(_HERE, "hostsim_contact.cpp"),
                                       os.path.join(_BUILD, f"libhostsim_contact_{key}.so"), _DEPS, defs))
        L.hostsim_contact.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_double, C.c_int,
                                      C.c_int64] + [C.c_void_p] * 5
        _libs[key] = L
    return _libs[key]


def lib_static(table):
    """the row on `table` as a compile-time table (built-in arms, compiled plugins)"""
    key, hdr = hostsim_build.table_header(_BUILD, table, "Tab_hostsim_contact")
    return _build(key, ["-include", hdr, "-DHOSTSIM_CONTACT_TAB=abrk::Tab_hostsim_contact"])


def lib_runtime(n):
    return _build(f"rt{n}", [f"-DHOSTSIM_CONTACT_RT_N={n}"])


def contact_step(table, q, dq, surface, frame="EE", offset=(0, 0, 0), vs=1e-3, tau=None, dtype=np.float64,
                 runtime=False):
    """-> (tau [B, n], report [B, 8]) of `dtype`.  surface: [B, S, 8]; tau: an array to ADD to (a copy is made), or None
    to write"""
    dt_ = np.dtype(dtype)
    n = int(table["n_joints"])
    q = np.ascontiguousarray(q, dtype=dt_)
    dq = np.ascontiguousarray(dq, dtype=dt_)
    s = np.ascontiguousarray(surface, dtype=dt_)
    B, S = s.shape[0], s.shape[1]
    assert q.shape == (B, n) and dq.shape == (B, n) and s.shape == (B, S, 8)
    acc = tau is not None
    out = np.array(tau, dtype=dt_, order="C") if acc else np.full((B, n), np.nan, dt_)
    rep = np.full((B, 8), np.nan, dt_)
    if runtime:
        L, desc = lib_runtime(n), _abi.desc_from_table(table)
        dp = C.cast(C.byref(desc), C.c_void_p)
    else:
        L, dp = lib_static(table), None
    assert L.hostsim_contact_n() == n
    off = (C.c_double * 3)(*[float(x) for x in offset])
    rc = L.hostsim_contact(dp, 0 if dt_ == np.float64 else 1, _abi.frame_id(frame, n), off, S, float(vs), int(acc), B,
                           q.ctypes.data, dq.ctypes.data, s.ctypes.data, out.ctypes.data, rep.ctypes.data)
    assert rc == 0, rc
    return out, rep
