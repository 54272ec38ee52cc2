"""The parity cases of the adaptive signal, shared by tests/test_adapt_hostsim.py and tests/test_adapt_gpu.py: seeded
populations and signals, and the fp64 reference run (tests/adapt_ref.py) of each case, computed once.

Signals: every input column is a sinusoid within +-0.8 with its own frequency and phase; the training signal is uniform
in +-30, redrawn at every tick; pes_learning_rate = 1e-4; intercepts uniform in +-0.9 (+-0.5 for the fp32 spiking cases,
which keeps the gains <= ~50; +-0.2 for the per-neuron fp32 spiking cases).

PATH_CASES are small cases that each reach a path of adapt_kernel, or a parameter, that the three parity shapes do not
(abr_control_amd/csrc/abrk_adapt.hip; a pass covers 256 V neurons, V = 16 / sizeof(T) when N % V == 0 and the arrays
are aligned, 1 otherwise):
  tiny_1, tiny_2  one lane; one 16-byte vector in fp64
  one_out         O = 1, odd D
  max_out         O = 16: all four groups of four outputs and the final reduction of lanes 8..15; D = 1; two passes with V = 1
  odd_all         a partial fourth group (O = 13); D = 13 takes the scalar encoder dot product in both types; N % 4 == 0
  max_in          D = 64, the whole first wavefront filters the input; a third group with one output (O = 9)
  passes64        three passes in fp64 with one active lane in the last (N = 1026 = 2 * 512 + 2); three ensembles (kappa
                  uses 342); nonzero initial weights; shift and scale
  passes32        three passes in fp32 with one active lane in the last (N = 2052 = 2 * 1024 + 4); D % 4 != 0
  taus0           a(0) = 1 for the input, training and output filters
  fast, slow      no refractory time; a refractory time of two steps"""
import functools

import numpy as np

from tests import adapt_ref

# (B, N, D, O, n_ensembles): a small one; N no multiple of 64 (nor of the 16-byte vectors) with a partial last wavefront
# of rows; the reference's default size in two ensembles (kappa uses 500)
PARITY_SHAPES = [(3, 100, 4, 2, 1), (70, 257, 12, 6, 1), (1, 1000, 14, 7, 2)]
PARITY_TICKS = 40
LEARNING_RATE = 1e-4
DT = 0.001
# fp32 spiking: (B, N, D, O, n_ensembles), ticks
F32_LIF_CASES = [((64, 32, 12, 6, 1), 30), ((64, 32, 4, 2, 1), 25)]
F32_BAND = 1e-4  # rows with a neuron-step this close to the threshold in fp64 are left out of the fp32 comparison
# fp32 spiking compared neuron by neuron: (B, N, D, O, n_ensembles), 30 ticks, intercepts within +-0.2, seeds 420..
F32_LIF_NEURON_SHAPES = [(4, 2052, 6, 3, 2), (4, 2052, 12, 6, 1), (3, 1028, 8, 16, 1)]
F32_LIF_NEURON_TICKS = 30

# name: (shape, ticks, seed, extras of Case); "draw" names what is drawn from RandomState(seed + 7), in this order
PATH_CASES = {
    "tiny_1": ((1, 1, 1, 1, 1), 40, 409, {}),
    "tiny_2": ((1, 2, 2, 1, 1), 40, 410, {}),
    "one_out": ((5, 64, 3, 1, 1), 40, 400, {}),
    "max_out": ((3, 300, 1, 16, 1), 40, 401, {}),
    "odd_all": ((3, 260, 13, 13, 1), 40, 402, dict(split=(12, 1))),
    "max_in": ((2, 130, 64, 9, 1), 40, 403, dict(split=(1, 63))),
    "passes64": ((2, 1026, 12, 12, 3), 40, 404, dict(split=(6, 6), draw=("shift", "scale", "W0"))),
    "passes32": ((2, 2052, 6, 3, 2), 30, 405, dict(draw=("shift", "scale"))),
    "taus0": ((4, 100, 4, 2, 1), 40, 406, dict(tau_input=0.0, tau_training=0.0, tau_output=0.0)),
    "fast": ((4, 100, 4, 2, 1), 40, 407, dict(dt=5e-4, tau_ref=0.0, tau_rc=0.01)),
    "slow": ((4, 100, 4, 2, 1), 40, 408, dict(dt=2e-3, tau_ref=4e-3)),
}
STATE = ("x_f", "e_f", "v", "ref", "a_f", "W", "out_f")


class Case:
    """split: (w0, w1), the widths in which a model wrapper hands the input to the tick as in0 and in1; shift, scale [D]
    and W0 [O, N] (the ensembles side by side): given, or named in `draw` and then drawn - shift uniform in +-0.3, scale
    in 0.5..1.5, W0 in +-1e-3 - from RandomState(seed + 7) in the order shift, scale, W0; params: dt, tau_input,
    tau_training, tau_output, tau_rc, tau_ref of the tick (the population's gains and biases keep Nengo's defaults)"""

    def __init__(self, shape, ticks, intercept_range, seed, split=None, shift=None, scale=None, W0=None, draw=(), **params):
        self.B, self.N, self.D, self.O, self.n_ens = shape
        self.n_per = self.N // self.n_ens
        self.ticks = ticks
        self.enc, self.gain, self.bias = adapt_ref.population(self.N, self.D, seed, intercept_range)
        rng = np.random.RandomState(seed + 1)
        freq = rng.uniform(2.0, 40.0, (self.B, self.D))
        phase = rng.uniform(0.0, 2 * np.pi, (self.B, self.D))
        t = np.arange(ticks)[:, None, None] * DT
        self.x = 0.8 * np.sin(2 * np.pi * freq * t + phase)  # [ticks, B, D]
        self.training = rng.uniform(-30.0, 30.0, (ticks, self.B, self.O))
        self.kw = dict(dt=DT, pes_learning_rate=LEARNING_RATE)
        unknown = set(params) - {"dt", "tau_input", "tau_training", "tau_output", "tau_rc", "tau_ref"}
        assert not unknown, unknown
        self.kw.update(params)
        assert split is None or (split[0] >= 1 and split[0] + split[1] == self.D)
        self.split = split
        rng = np.random.RandomState(seed + 7)
        draws = {"shift": lambda: rng.uniform(-0.3, 0.3, self.D), "scale": lambda: rng.uniform(0.5, 1.5, self.D),
                 "W0": lambda: rng.uniform(-1e-3, 1e-3, (self.O, self.N))}
        self.tables = dict(shift=shift, scale=scale, W0=W0)  # what AdaptRef and HostAdapt take beside kw
        for name in ("shift", "scale", "W0"):  # (the order of the draws)
            if name in draw:
                assert self.tables[name] is None, name
                self.tables[name] = draws[name]()
        self.shift, self.scale, self.W0 = (self.tables[k] for k in ("shift", "scale", "W0"))

    def run(self, model, rows=slice(None), ticks=None):
        """tick `model` (AdaptRef, HostAdapt, GpuAdapt: anything with tick(x, training)) through the case, or through its
        first `ticks` ticks -> outs [ticks, B, O].  The model gets the unsplit x."""
        return np.stack([model.tick(self.x[k, rows], self.training[k, rows])
                         for k in range(self.ticks if ticks is None else ticks)])


def state_errors(ref_state, got_state, rows=slice(None), neurons=None):
    """{name: error} of the state arrays of `got_state` (those it holds) against the reference's: the largest
    |difference| over max(largest |reference value|, 1) for v, ref, a_f, x_f, e_f and out_f, and over the largest |W|
    for W (over 1 if the reference's weights are all zero).  rows: the rows to compare; neurons: a mask [B, N] of the
    neurons to compare in v, ref, a_f and W (the others count neither in the difference nor in the largest value)."""
    errs = {}
    for k in STATE:
        if got_state.get(k) is None:
            continue
        want, got = np.asarray(ref_state[k], dtype=np.float64)[rows], np.asarray(got_state[k], dtype=np.float64)[rows]
        assert want.shape == got.shape, (k, want.shape, got.shape)
        if neurons is not None and k in ("v", "ref", "a_f", "W"):
            m = neurons[rows] if k != "W" else np.broadcast_to(neurons[rows][:, None, :], want.shape)
            want, got = want[m], got[m]
        top = np.abs(want).max() if want.size else 0.0
        den = (top if top > 0 else 1.0) if k == "W" else max(top, 1.0)
        errs[k] = np.abs(got - want).max() / den if want.size else 0.0
    return errs


def out_error(outs, got, rows=slice(None)):
    """the largest |difference| of every tick's output over the largest |reference output| (over 1 if all are zero)"""
    want = outs[:len(got), rows]
    top = np.abs(want).max()
    return np.abs(np.asarray(got, dtype=np.float64)[:, rows] - want).max() / (top if top > 0 else 1.0)


@functools.lru_cache(maxsize=None)
def reference_model(kind, index, neuron_type):
    """-> (case, outs [ticks, B, O], the AdaptRef after the case's last tick) of the fp64 reference; kind: "parity" |
    "f32lif" | "f32lif_n" (index: a number) | "path" (index: a name of PATH_CASES).  Cached: the arrays are shared, leave
    them unchanged."""
    if kind == "parity":
        case = Case(PARITY_SHAPES[index], PARITY_TICKS, 0.9, 100 + index)
    elif kind == "f32lif":
        shape, ticks = F32_LIF_CASES[index]
        case = Case(shape, ticks, 0.5, 200 + index)
    elif kind == "f32lif_n":
        case = Case(F32_LIF_NEURON_SHAPES[index], F32_LIF_NEURON_TICKS, 0.2, 420 + index)
    else:
        shape, ticks, seed, extras = PATH_CASES[index]
        case = Case(shape, ticks, 0.9, seed, **extras)
    ref = adapt_ref.AdaptRef(case.enc, case.gain, case.bias, case.B, case.O, case.n_per, neuron_type, band=F32_BAND,
                             **case.tables, **case.kw)
    outs = case.run(ref)
    return case, outs, ref


def reference(kind, index, neuron_type):
    """-> (case, outs [ticks, B, O], final state dict, near [B], margin [B]) of reference_model"""
    case, outs, ref = reference_model(kind, index, neuron_type)
    return case, outs, ref.state(), ref.near, ref.margin
