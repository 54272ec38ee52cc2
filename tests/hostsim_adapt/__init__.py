"""Python side of the hostsim_adapt TEST AID (tests/hostsim_adapt/hostsim_adapt.cpp): the adaptive signal's row program
built for the host on first use.  Never imported by the product."""
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
    so = hostsim_build.build(os.path.join(_HERE, "hostsim_adapt.cpp"),
                             os.path.join(_HERE, "build", "libhostsim_adapt.so"), hostsim_build.csrc("abrk_adapt.h"))
    L = C.CDLL(so)
    L.hostsim_adapt_step.argtypes = [C.c_int] * 7 + [C.c_double] * 7 + [C.c_int64] + [C.c_void_p] * 17
    _lib = L
    return L


class HostAdapt:
    """B rows of the adaptive signal stepped by the host build, with the constructor and tick() of adapt_ref.AdaptRef.
    split: (w0, w1) - tick() then hands its x_in to the row program in two arrays, in0 [B,w0] and in1 [B,w1]"""

    def __init__(self, enc, gain, bias, B, n_output, n_per, neuron_type="lif", shift=None, scale=None, dt=0.001,
                 tau_input=0.012, tau_training=0.012, tau_output=0.2, tau_rc=0.02, tau_ref=0.002,
                 pes_learning_rate=1e-6, W0=None, split=None):
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        self.enc, self.gain, self.bias = f8(enc), f8(gain), f8(bias)
        N, D = self.enc.shape
        self.shift = np.zeros(D) if shift is None else f8(shift)
        self.scale = np.ones(D) if scale is None else f8(scale)
        self.head = ({"lif": 0, "lif_rate": 1}[neuron_type], D, n_output, N, n_per)
        self.taus = (dt, tau_input, tau_training, tau_output, tau_rc, tau_ref, pes_learning_rate)
        O, self.B = n_output, B
        self.split = split
        self.st = {"x_f": np.zeros((B, D)), "e_f": np.zeros((B, O)), "v": np.zeros((B, N)), "ref": np.zeros((B, N)),
                   "a_f": np.zeros((B, N)), "W": np.zeros((B, O, N)), "out_f": np.zeros((B, O))}
        if W0 is not None:
            self.st["W"][:] = W0

    def state(self):
        return self.st

    def tick(self, x_in, training, in1=None, u_add=None):
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        if self.split is not None and in1 is None:
            x_in, in1 = np.asarray(x_in)[:, :self.split[0]], np.asarray(x_in)[:, self.split[0]:]
        x_in, training = f8(x_in), f8(training)
        in1 = None if in1 is None else f8(in1)
        out = np.zeros((self.B, self.head[2]))
        p = lambda a: None if a is None else a.ctypes.data
        lib().hostsim_adapt_step(*self.head, x_in.shape[1], 0 if in1 is None else in1.shape[1], *self.taus, self.B,
                                 p(self.enc), p(self.gain), p(self.bias), p(self.shift), p(self.scale), p(x_in), p(in1),
                                 p(training), *(p(self.st[k]) for k in ("x_f", "e_f", "v", "ref", "a_f", "W", "out_f")),
                                 p(out), p(u_add))
        return out
