"""Does the adaptive signal learn?  One population of 1000 neurons over a constant 4-dimensional input has to produce
d = (5, -3): the training signal is d - out of the previous tick, pes_learning_rate = 1e-3, tau_output = 0.01, 1500
ticks.  Run on the NumPy statement (tests/adapt_ref.py), on the host build of the row program (tests/hostsim_adapt) and,
through DynamicsAdaptation.generate(), on the GPU.

  lif_rate: |out - d| <= 1e-3 |d| from tick 600 on (a model of this tick gave 1.6e-5 at tick 600, 1e-9 at tick 1000)
  lif:      |out - d| <= 0.2 in every tick after 300 (the model's worst was 0.098: the spiking noise of one arm's 1000
            neurons sets it, hence the factor two)

|.| is the Euclidean norm over the two outputs."""
import numpy as np
import pytest

from tests import adapt_ref

N, D, O, TICKS = 1000, 4, 2, 1500
TARGET = np.array([5.0, -3.0])
X = np.array([0.3, -0.2, 0.5, 0.1])
SEED = 7
KW = dict(dt=0.001, pes_learning_rate=1e-3, tau_output=0.01)


def _closed_loop(tick):
    """tick(x [1,D], training [1,O]) -> out [1,O];  -> |out - d| of every tick"""
    out, err = np.zeros((1, O)), np.zeros(TICKS)
    for k in range(TICKS):
        out = tick(X[None, :], TARGET[None, :] - out)
        err[k] = np.linalg.norm(out[0] - TARGET)
    return err


def _check(err, neuron_type, who):
    if neuron_type == "lif_rate":
        print(f"{who} lif_rate: |out - d| at tick 600 {err[600]:.2e}, worst from 600 on {err[600:].max():.2e}, "
              f"at tick 1000 {err[1000]:.2e}")
        assert err[600:].max() <= 1e-3 * np.linalg.norm(TARGET)
    else:
        print(f"{who} lif: worst |out - d| after tick 300 {err[301:].max():.3f}")
        assert err[301:].max() <= 0.2


def _model(cls, neuron_type):
    enc, gain, bias = adapt_ref.population(N, D, SEED)
    return cls(enc, gain, bias, 1, O, N, neuron_type, **KW)


@pytest.mark.parametrize("neuron_type", ["lif_rate", "lif"])
def test_numpy_reference_learns(neuron_type):
    _check(_closed_loop(_model(adapt_ref.AdaptRef, neuron_type).tick), neuron_type, "adapt_ref")


@pytest.mark.parametrize("neuron_type", ["lif_rate", "lif"])
def test_host_build_learns(neuron_type):
    from tests import hostsim_adapt

    _check(_closed_loop(_model(hostsim_adapt.HostAdapt, neuron_type).tick), neuron_type, "host build")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("neuron_type", ["lif_rate", "lif"])
def test_generate_learns_on_the_gpu(neuron_type, dtype):
    from abr_control_amd.controllers.signals import DynamicsAdaptation

    enc, intercepts, max_rates = adapt_ref.population_parts(N, D, SEED)
    adapt = DynamicsAdaptation(D, O, n_neurons=N, intercepts=intercepts, encoders=enc, max_rates=max_rates,
                               neuron_type=neuron_type, dtype=dtype, **KW)
    _check(_closed_loop(adapt.generate), neuron_type, f"generate() {np.dtype(dtype).name}")
    W = adapt.get_weights()
    assert len(W) == 1 and W[0].shape == (1, O, N) and np.abs(W[0]).max() > 0
