"""Nonlinear dynamics adaptation (abr_control/controllers/signals/dynamics_adaptation.py:7-266) for one arm or a batch:
ensembles of LIF neurons over the scaled joint state whose decoders learn by PES from the controller's training signal.
The reference builds a Nengo network and steps its simulator; here one kernel launch (engine.adapt_step) advances every
row's population by one tick, with all state in device memory."""
import numpy as np

from ... import _abi, engine
from ..._lib import DeviceArray


def cosine_similarity_ppf(dimensions, y):
    """nengo.dists.CosineSimilarity(dimensions).ppf(y): the inverse CDF of the dot product of two random unit vectors"""
    try:
        from scipy.special import betaincinv
    except ImportError as e:
        raise ImportError("the default intercepts of DynamicsAdaptation need scipy.special.betaincinv: install scipy "
                          "or pass `intercepts`") from e
    y = np.asarray(y, dtype=float)
    x = np.sqrt(betaincinv(0.5, (dimensions - 1) / 2.0, np.abs(y * 2 - 1)))
    return np.where(y > 0.5, x, -x)


class DynamicsAdaptation:
    """The reference's constructor arguments, in its order and with its defaults, then the additions of this package:

    neuron_type: "lif" (spiking, the reference's default) or "lif_rate"
    max_rates: (n_ensembles, n_neurons) firing rates at enc . x = 1; default: uniform on 200..400 Hz from `seed`, Nengo's
        Ensemble default
    dtype, device, stream: the arithmetic and placement of the kernel

    generate(input_signal, training_signal) takes (n,) like the reference or (B, n) for B independent populations with
    the same encoders, gains and biases and their own state and weights; the state is allocated at the first call.

    Differences from the reference: the default encoders are seeded random unit vectors (the reference scatters them
    with a quasi-random sequence that needs Nengo), `spherical=True` is not built (its transform is a per-tick inverse
    incomplete beta function), and the tick is Nengo's published Lowpass, LIF and PES operators in this package's own
    order (include/abrk.h, abrk_adapt_step_batch) - agreement with Nengo's simulator to the tick is not claimed."""

    tau_rc, tau_ref = 0.02, 0.002  # Nengo's LIF defaults

    def __init__(self, n_input, n_output, n_neurons=1000, n_ensembles=1, seed=None, pes_learning_rate=1e-6,
                 intercepts=None, weights=None, encoders=None, spherical=False, means=None, variances=None,
                 tau_input=0.012, tau_training=0.012, tau_output=0.2, dt=0.001, neuron_type="lif", max_rates=None,
                 dtype=np.float64, device=0, stream=None):
        if spherical:
            raise NotImplementedError("spherical=True (the hypersphere projection of the inputs, "
                                      "dynamics_adaptation.py:242-249) is not built")
        self.dt = dt
        self.n_input, self.n_output = int(n_input), int(n_output)
        self.n_neurons, self.n_ensembles = int(n_neurons), int(n_ensembles)
        self.spherical = False
        # dynamics_adaptation.py:86-93: one of the two given -> the other has no effect
        if means is not None and variances is None:
            variances = np.ones(np.shape(means))
        elif means is None and variances is not None:
            means = np.zeros(np.shape(variances))
        self.means = None if means is None else np.asarray(means, dtype=float)
        self.variances = None if variances is None else np.asarray(variances, dtype=float)
        self.tau_input, self.tau_training, self.tau_output = tau_input, tau_training, tau_output
        self.seed = seed
        self.pes_learning_rate = pes_learning_rate
        self.neuron_type = neuron_type
        self.dtype, self.device, self.stream = np.dtype(dtype), device, stream
        N, D, O = self.n_neurons * self.n_ensembles, self.n_input, self.n_output
        rng = np.random.RandomState(seed)
        triangular = rng.triangular(left=0.35, mode=0.45, right=0.55, size=N)  # dynamics_adaptation.py:111-113
        default_rates = rng.uniform(200.0, 400.0, size=N)
        default_encoders = rng.standard_normal((N, D))
        if intercepts is None:
            intercepts = cosine_similarity_ppf(D + 2, 1 - triangular)
        self.intercepts = np.asarray(intercepts, dtype=float).reshape(self.n_ensembles, self.n_neurons)
        self.max_rates = np.asarray(default_rates if max_rates is None else max_rates, dtype=float).reshape(
            self.n_ensembles, self.n_neurons)
        if weights is None:
            weights = np.zeros((self.n_ensembles, O, self.n_neurons))
        self.weights = np.asarray(weights, dtype=float).reshape(self.n_ensembles, O, self.n_neurons)
        enc = np.asarray(default_encoders if encoders is None else encoders, dtype=float).reshape(N, D)
        self.encoders = (enc / np.linalg.norm(enc, axis=1, keepdims=True)).reshape(self.n_ensembles, self.n_neurons, D)
        self.gain, self.bias = _abi.lif_gain_bias(self.intercepts.reshape(N), self.max_rates.reshape(N), self.tau_rc,
                                                  self.tau_ref)
        self.params = _abi.make_adapt_params(D, O, self.n_neurons, self.n_ensembles, neuron_type, dt, tau_input,
                                             tau_training, tau_output, self.tau_rc, self.tau_ref, pes_learning_rate)
        if not 1 <= D <= _abi.ADAPT_MAX_INPUT or not 1 <= O <= _abi.ADAPT_MAX_OUTPUT or N < 1:
            raise ValueError(f"n_input 1..{_abi.ADAPT_MAX_INPUT}, n_output 1..{_abi.ADAPT_MAX_OUTPUT} and at least one "
                             f"neuron, got {D}, {O}, {N}")
        self.B = None
        self.state = None

    def _W0(self):
        """the initial weights as one [O, N] block, the ensembles side by side"""
        return np.concatenate(list(self.weights), axis=1)

    def _allocate(self, B):
        D = self.n_input
        dev = lambda a: DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=self.dtype), self.device, engine._sp(self.stream))
        shift = np.zeros(D) if self.means is None else np.broadcast_to(self.means, (D,))
        scale = np.ones(D) if self.variances is None else 1.0 / np.broadcast_to(self.variances, (D,))
        self._tables = [dev(self.encoders.reshape(-1, D)), dev(self.gain), dev(self.bias), dev(shift), dev(scale)]
        self.state = {k: DeviceArray(sh, self.dtype, self.device)
                      for k, sh in engine.adapt_state_shapes(self.params, B).items()}
        self._in = DeviceArray((B, D), self.dtype, self.device)
        self._training = DeviceArray((B, self.n_output), self.dtype, self.device)
        self._out = DeviceArray((B, self.n_output), self.dtype, self.device)
        self.B = B
        self.reset()

    def _rows(self, B):
        if self.B is None:
            self._allocate(int(B))
        elif int(B) != self.B:
            raise ValueError(f"this DynamicsAdaptation holds the state of {self.B} rows; got a batch of {B}")

    def reset(self):
        """back to the initial weights, with every filter, voltage and refractory time at zero"""
        if self.state is None:
            return
        for k, arr in self.state.items():
            if k == "W":
                arr.copy_from_numpy(np.broadcast_to(self._W0(), arr.shape), self.stream)
            else:
                arr.zero_(self.stream)

    def scale_inputs(self, input_signal):
        """(input_signal - means) / variances (dynamics_adaptation.py:240): what the kernel applies to its inputs"""
        x = np.asarray(input_signal, dtype=float)
        if self.means is None:
            return x
        return (x - self.means) / self.variances

    def generate(self, input_signal, training_signal):
        """One tick: input_signal (n_input,) or (B, n_input) - unscaled, as the reference takes it - and training_signal
        (n_output,) or (B, n_output) -> the adaptive signal, of the same shape as training_signal."""
        x = np.asarray(input_signal, dtype=self.dtype)
        t = np.asarray(training_signal, dtype=self.dtype)
        single = t.ndim == 1
        x = x.reshape(1, -1) if single else x
        t = t.reshape(1, -1) if single else t
        if x.shape[1:] != (self.n_input,) or t.shape != (x.shape[0], self.n_output):
            raise ValueError(f"expected [B, {self.n_input}] and [B, {self.n_output}], got {x.shape} and {t.shape}")
        self._rows(x.shape[0])
        self._in.copy_from_numpy(x, self.stream)
        self._training.copy_from_numpy(t, self.stream)
        self.step(self._in, None, self._training, out=self._out)
        out = self._out.numpy(self.stream)
        return out[0] if single else out

    def step(self, q, dq, training, u_add=None, out=None):
        """One tick on DeviceArrays, enqueued on this object's stream - what a recorded loop calls inside its Plan: the
        input is concat(q, dq) (dq None: q alone is the whole input), `training` the law's training_signal; the output is
        added to u_add [B, n_output] when given.  -> out (a DeviceArray; this object's own buffer when none is given,
        so that a recorded tick never writes to an array the caller dropped)."""
        self._rows(q.shape[0])
        out = self._out if out is None else out
        return engine.adapt_step(self.params, *self._tables, q, training, self.state, in1=dq, out=out, u_add=u_add,
                                 dtype=self.dtype, device=self.device, stream=self.stream)

    def get_weights(self):
        """the current decoders: a list with one [B, n_output, n_neurons] array per ensemble"""
        if self.state is None:
            raise RuntimeError("no state yet: the first generate() / step() allocates it")
        W = self.state["W"].numpy(self.stream)
        return [W[:, :, e * self.n_neurons:(e + 1) * self.n_neurons].copy() for e in range(self.n_ensembles)]
