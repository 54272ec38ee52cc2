"""The parity cases of the adaptive signal, shared by tests/test_adapt_hostsim.py and tests/test_adapt_gpu.py: seeded
populations and signals, and the fp64 reference run (tests/adapt_ref.py) of each case, computed once.

Signals: every input column is a sinusoid within +-0.8 with its own frequency and phase; the training signal is uniform
in +-30, redrawn at every tick; pes_learning_rate = 1e-4; intercepts uniform in +-0.9 (+-0.5 for the fp32 spiking cases,
which keeps the gains <= ~50)."""
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


class Case:
    def __init__(self, shape, ticks, intercept_range, seed):
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

    def run(self, model, rows=slice(None)):
        """tick `model` (AdaptRef, HostAdapt: anything with tick(x, training)) through the case -> outs [ticks, B, O]"""
        return np.stack([model.tick(self.x[k, rows], self.training[k, rows]) for k in range(self.ticks)])


@functools.lru_cache(maxsize=None)
def reference(kind, index, neuron_type):
    """-> (case, outs [ticks, B, O], final state dict, near [B], margin [B]) of the fp64 reference; kind: "parity" | "f32lif".
    Cached: the arrays are shared, leave them unchanged."""
    if kind == "parity":
        case = Case(PARITY_SHAPES[index], PARITY_TICKS, 0.9, 100 + index)
    else:
        shape, ticks = F32_LIF_CASES[index]
        case = Case(shape, ticks, 0.5, 200 + index)
    ref = adapt_ref.AdaptRef(case.enc, case.gain, case.bias, case.B, case.O, case.n_per, neuron_type, band=F32_BAND,
                             **case.kw)
    outs = case.run(ref)
    return case, outs, ref.state(), ref.near, ref.margin
