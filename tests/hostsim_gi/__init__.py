"""Python side of the hostsim_gi TEST AID (tests/hostsim_gi/hostsim_gi.cpp): the row programs built for the host on a
general-inertia arm table, one small library per table.  Never imported by the product."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

from abr_control_amd import _abi
from abr_control_amd.engine import _OUT_SHAPES, _WANT_BITS

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "abr_control_amd", "csrc")
_BUILD = os.path.join(_HERE, "build")
_libs = {}


def _sources():
    return [os.path.join(_HERE, "hostsim_gi.cpp")] + [
        os.path.join(_CSRC, f) for f in ("abrk_device.h", "abrk_ctrl.h", "abrk_rows.h", "abrk_arms_builtin.h",
                                         "abrk_sincos_table.h")]


def lib_for(table):
    """the host build of the row programs on `table` (built on first use, rebuilt when a source is newer)"""
    src = _abi.render_tab_struct(table, "Tab_hostsim_gi")
    key = hashlib.sha256(src.encode()).hexdigest()[:16]
    if key in _libs:
        return _libs[key]
    os.makedirs(_BUILD, exist_ok=True)
    hdr = os.path.join(_BUILD, f"tab_{key}.h")
    so = os.path.join(_BUILD, f"libhostsim_gi_{key}.so")
    with open(hdr + ".tmp", "w") as fh:
        fh.write("#pragma once\nnamespace abrk {\n" + src + "\n}  // namespace abrk\n")
    os.replace(hdr + ".tmp", hdr)
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in _sources()):
        r = subprocess.run(
            ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-shared",
             "-fno-signed-zeros", "-ffinite-math-only", "--cuda-host-only", "-include", hdr,
             "-DHOSTSIM_GI_TAB=abrk::Tab_hostsim_gi", "-o", so + ".tmp", _sources()[0]],
            capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError("hostsim_gi build failed:\n" + r.stderr[-3000:])
        os.replace(so + ".tmp", so)
    _libs[key] = C.CDLL(so)
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
