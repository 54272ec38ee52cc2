"""NumPy statement of one tick of the adaptive signal (include/abrk.h, abrk_adapt_step_batch) - TEST AID, fp64,
vectorised over the rows.  The tick has no counterpart that can be run here (the reference's DynamicsAdaptation steps
a Nengo simulator), so the kernels are pinned to this restatement of the published operators - Lowpass, Nengo's LIF
and LIFRate steps, PES - written from the equations and not from the row program.

With a(tau) = 1 - exp(-dt / tau), a(0) = 1:
  1  x = (in - shift) * scale;  x_f += a(tau_input) (x - x_f)
  2  e_f += a(tau_training) (training - e_f)
  3  J = gain (enc . x_f) + bias;  s = LIF step | LIFRate
  4  y = W s                                   (weights from before this tick's update)
  5  out_f += a(tau_output) (y - out_f)
  6  a_f += a(tau_pre) (s - a_f),  tau_pre = 0.005
  7  W += (pes_learning_rate dt / n_per) e_f (x) a_f

Besides the outputs it keeps, per row, how close the spiking decision v > 1 ever came to a tie: the number of
neuron-steps with |v - 1| < band and the smallest |v - 1| seen, and per neuron whether any of its steps had
|v - 1| < band (near_n) - rows, neurons and cases where another arithmetic may decide differently are recognised by
them."""
import numpy as np

TAU_PRE = 0.005


def lowpass_gain(dt, tau):
    return 1.0 - np.exp(-dt / tau) if tau > 0 else 1.0


class AdaptRef:
    def __init__(self, enc, gain, bias, B, n_output, n_per, neuron_type="lif", shift=None, scale=None, dt=0.001,
                 tau_input=0.012, tau_training=0.012, tau_output=0.2, tau_rc=0.02, tau_ref=0.002,
                 pes_learning_rate=1e-6, W0=None, band=1e-4):
        self.enc = np.asarray(enc, dtype=np.float64)
        N, D = self.enc.shape
        self.gain, self.bias = np.asarray(gain, dtype=np.float64), np.asarray(bias, dtype=np.float64)
        self.shift = np.zeros(D) if shift is None else np.asarray(shift, dtype=np.float64)
        self.scale = np.ones(D) if scale is None else np.asarray(scale, dtype=np.float64)
        assert neuron_type in ("lif", "lif_rate")
        self.lif = neuron_type == "lif"
        self.dt, self.tau_rc, self.tau_ref = dt, tau_rc, tau_ref
        self.a_in, self.a_tr = lowpass_gain(dt, tau_input), lowpass_gain(dt, tau_training)
        self.a_out, self.a_pre = lowpass_gain(dt, tau_output), lowpass_gain(dt, TAU_PRE)
        self.kappa = pes_learning_rate * dt / n_per
        O = n_output
        self.x_f, self.e_f, self.out_f = np.zeros((B, D)), np.zeros((B, O)), np.zeros((B, O))
        self.v, self.ref, self.a_f = np.zeros((B, N)), np.zeros((B, N)), np.zeros((B, N))
        self.W = np.zeros((B, O, N)) if W0 is None else np.broadcast_to(np.asarray(W0, dtype=np.float64), (B, O, N)).copy()
        self.band = band
        self.near = np.zeros(B, dtype=np.int64)  # neuron-steps with |v - 1| < band
        self.margin = np.full(B, np.inf)         # smallest |v - 1| at a threshold decision
        self.near_n = np.zeros((B, N), dtype=bool)  # neurons with any step at which |v - 1| < band

    def state(self):
        return {"x_f": self.x_f, "e_f": self.e_f, "v": self.v, "ref": self.ref, "a_f": self.a_f, "W": self.W,
                "out_f": self.out_f}

    def _spikes(self, J):
        dt = self.dt
        self.ref -= dt
        delta = np.clip(dt - self.ref, 0.0, dt)
        self.v -= (J - self.v) * np.expm1(-delta / self.tau_rc)
        gap = np.abs(self.v - 1.0)
        self.near += np.sum(gap < self.band, axis=1)
        self.near_n |= gap < self.band
        self.margin = np.minimum(self.margin, gap.min(axis=1))
        spiked = self.v > 1.0
        over, den = self.v - 1.0, J - 1.0
        # no infinity is formed: the overshoot of a voltage that rose towards J lies below J - 1; anything else, and a
        # quotient that rounds to 1, counts as no overshoot
        ok = spiked & (den > over)
        r = np.where(ok, over / np.where(ok, den, 1.0), 0.0)
        r = np.where(r < 1.0, r, 0.0)
        t_s = dt + self.tau_rc * np.log1p(-r)
        self.v = np.where(spiked, 0.0, np.maximum(self.v, 0.0))
        self.ref = np.where(spiked, self.tau_ref + t_s, self.ref)
        return spiked / dt

    def _rates(self, J):
        on = J > 1.0
        jm = np.where(on, J - 1.0, 1.0)
        return np.where(on, 1.0 / (self.tau_ref + self.tau_rc * np.log1p(1.0 / jm)), 0.0)

    def tick(self, x_in, training):
        """x_in [B,D] (unscaled), training [B,O] -> out [B,O] (a copy)"""
        x = (np.asarray(x_in, dtype=np.float64) - self.shift) * self.scale
        self.x_f += self.a_in * (x - self.x_f)
        self.e_f += self.a_tr * (np.asarray(training, dtype=np.float64) - self.e_f)
        J = self.gain * (self.x_f @ self.enc.T) + self.bias
        s = self._spikes(J) if self.lif else self._rates(J)
        y = np.einsum("bon,bn->bo", self.W, s)
        self.out_f += self.a_out * (y - self.out_f)
        self.a_f += self.a_pre * (s - self.a_f)
        self.W += self.kappa * self.e_f[:, :, None] * self.a_f[:, None, :]
        return self.out_f.copy()


def population_parts(N, D, seed, intercept_range=0.9):
    """a seeded test population -> unit encoders [N,D], intercepts uniform in +-intercept_range, max rates uniform on
    200..400"""
    rng = np.random.RandomState(seed)
    enc = rng.standard_normal((N, D))
    enc /= np.linalg.norm(enc, axis=1, keepdims=True)
    return enc, rng.uniform(-intercept_range, intercept_range, N), rng.uniform(200.0, 400.0, N)


def population(N, D, seed, intercept_range=0.9):
    """population_parts -> enc [N,D], gain [N], bias [N] by Nengo's LIF closed form"""
    enc, intercepts, max_rates = population_parts(N, D, seed, intercept_range)
    tau_rc, tau_ref = 0.02, 0.002
    x = 1.0 / (1.0 - np.exp((tau_ref - 1.0 / max_rates) / tau_rc))
    gain = (1.0 - x) / (intercepts - 1.0)
    return enc, gain, 1.0 - gain * intercepts
