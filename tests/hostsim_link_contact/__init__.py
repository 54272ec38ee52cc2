"""Python side of the hostsim_link_contact TEST AID (tests/hostsim_link_contact/hostsim_link_contact.cpp): the row
program of the whole-arm contact (link_contact_body) built for the host, one small library per arm table (compile-time
tables) or per joint count (runtime tables).  Never imported by the product."""
import ctypes as C
import os

import numpy as np

from abr_control_amd import _abi
from tests import hostsim_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_BUILD = os.path.join(_HERE, "build")
_DEPS = hostsim_build.csrc("abrk_device.h", "abrk_ctrl.h", "abrk_rows.h", "abrk_link_contact.h", "abrk_rt.h",
                           "abrk_arms_builtin.h", "abrk_sincos_table.h") + [hostsim_build.ABRK_H]
_libs = {}


def _build(key, defs):
    if key not in _libs:
        L = C.CDLL(hostsim_build.build(os.path.join(_HERE, "hostsim_link_contact.cpp"),
                                       os.path.join(_BUILD, f"libhostsim_link_contact_{key}.so"), _DEPS, defs))
        L.hostsim_link_contact.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_int,
                                           C.c_int64] + [C.c_void_p] * 5
        _libs[key] = L
    return _libs[key]


def lib_static(table):
    """the row on `table` as a compile-time table (built-in arms, compiled plugins)"""
    key, hdr = hostsim_build.table_header(_BUILD, table, "Tab_hostsim_link_contact")
    return _build(key, ["-include", hdr, "-DHOSTSIM_LINK_CONTACT_TAB=abrk::Tab_hostsim_link_contact"])


def lib_runtime(n):
    return _build(f"rt{n}", [f"-DHOSTSIM_LINK_CONTACT_RT_N={n}"])


def link_contact_step(table, q, dq, obstacle, radius, vs=1e-3, tau=None, dtype=np.float64, runtime=False):
    """-> (tau [B, n], report [B, 8]) of `dtype`.  obstacle: [B, K, 7]; radius: [n]; tau: an array to ADD to (a copy is
    made), or None to write"""
    dt_ = np.dtype(dtype)
    n = int(table["n_joints"])
    q = np.ascontiguousarray(q, dtype=dt_)
    dq = np.ascontiguousarray(dq, dtype=dt_)
    s = np.ascontiguousarray(obstacle, dtype=dt_)
    B, K = s.shape[0], s.shape[1]
    assert q.shape == (B, n) and dq.shape == (B, n) and s.shape == (B, K, 7)
    acc = tau is not None
    out = np.array(tau, dtype=dt_, order="C") if acc else np.full((B, n), np.nan, dt_)
    rep = np.full((B, 8), np.nan, dt_)
    if runtime:
        L, desc = lib_runtime(n), _abi.desc_from_table(table)
        dp = C.cast(C.byref(desc), C.c_void_p)
    else:
        L, dp = lib_static(table), None
    assert L.hostsim_link_contact_n() == n
    rad = (C.c_double * n)(*[float(x) for x in np.broadcast_to(radius, (n,))])
    rc = L.hostsim_link_contact(dp, 0 if dt_ == np.float64 else 1, K, rad, float(vs), int(acc), B, q.ctypes.data,
                                dq.ctypes.data, s.ctypes.data, out.ctypes.data, rep.ctypes.data)
    assert rc == 0, rc
    return out, rep
