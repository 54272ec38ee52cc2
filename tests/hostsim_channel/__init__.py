"""Python side of the hostsim_channel TEST AID (tests/hostsim_channel/hostsim_channel.cpp): the measurement channel's row
program built for the host on first use.  Never imported by the product."""
import ctypes as C
import os

import numpy as np

from tests import hostsim_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = hostsim_build.build(os.path.join(_HERE, "hostsim_channel.cpp"),
                             os.path.join(_HERE, "build", "libhostsim_channel.so"),
                             hostsim_build.csrc("abrk_channel.h"))
    L = C.CDLL(so)
    L.hostsim_channel_step.argtypes = [C.c_int] * 3 + [C.c_int64, C.c_uint64, C.c_int64, C.c_double, C.c_double] + [
        C.c_void_p] * 12
    L.hostsim_channel_normal.restype = C.c_double
    L.hostsim_channel_normal.argtypes = [C.c_uint64, C.c_int64, C.c_uint32, C.c_uint32, C.c_void_p]
    L.hostsim_channel_philox.restype = None
    L.hostsim_channel_philox.argtypes = [C.c_void_p] * 3
    _lib = L
    return L


def philox(counter, key):
    c, k, out = np.array(counter, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
    lib().hostsim_channel_philox(c.ctypes.data, k.ctypes.data, out.ctypes.data)
    return out


def normal(seed, row, tick, col):
    """-> (the four Philox words, n)"""
    w = np.zeros(4, np.uint32)
    n = lib().hostsim_channel_normal(seed, row, tick, col, w.ctypes.data)
    return w, n


class HostChannel:
    """B rows of the channel stepped by the host build in fp64, with the constructor and tick() of
    channel_ref.ChannelRef"""

    def __init__(self, width, B, bias=0.0, sigma=0.0, resolution=0.0, delay=0, difference=False, tau_diff=0.0, dt=0.001,
                 seed=0, row_offset=0, w0=None):
        col = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (width,)).copy()
        self.W, self.B, self.d, self.difference = width, B, int(delay), difference
        self.w0 = width if w0 is None else w0
        self.cols = (col(bias), col(sigma), col(resolution))
        self.head = (int(seed), int(row_offset), float(dt), float(tau_diff))
        self.counter = np.zeros(B, np.int32)
        # NaN where the tick must not read before it has written
        self.ring = np.full((self.d + 1, B, width), np.nan) if self.d else None
        self.prev = np.full((B, width), np.nan) if difference else None
        self.d_f = np.full((B, width), np.nan) if difference else None

    def tick(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        w0, w1 = self.w0, self.W - self.w0
        in0, in1 = np.ascontiguousarray(x[:, :w0]), (np.ascontiguousarray(x[:, w0:]) if w1 else None)
        out0, out1 = np.empty((self.B, w0)), (np.empty((self.B, w1)) if w1 else None)
        dy = np.empty((self.B, self.W)) if self.difference else None
        p = lambda a: None if a is None else a.ctypes.data
        lib().hostsim_channel_step(w0, w1, self.d, self.B, *self.head, *(p(c) for c in self.cols), p(in0), p(in1),
                                   p(out0), p(out1), p(dy), p(self.counter), p(self.ring), p(self.prev), p(self.d_f))
        return (out0 if out1 is None else np.concatenate([out0, out1], axis=1)), dy
