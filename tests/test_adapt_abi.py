"""The adaptive signal without a GPU: every ABRK_EINVAL case of abrk_adapt_step_batch (the checks come before the device
is touched), and the Python surface of controllers.signals.DynamicsAdaptation - the reference's constructor arguments,
Nengo's closed form of gain and bias, what is refused."""
import ctypes as C
import inspect

import numpy as np
import pytest

from abr_control_amd import _abi
from abr_control_amd._lib import lib
from abr_control_amd.controllers.signals import DynamicsAdaptation

D, O, N, B = 4, 2, 8, 3


def _call(dtype=_abi.F64, B_=B, w0=D, w1=0, null=(), state_null=(), params=True, state=True, **changes):
    """the entry point on host arrays with one thing wrong -> (return code, message)"""
    kw = dict(n_input=D, n_output=O, n_neurons=N, n_ensembles=1, neuron_type="lif")
    p = _abi.make_adapt_params(**kw)
    for k, v in changes.items():
        setattr(p, k, v)
    arr = {k: np.zeros(s) for k, s in dict(enc=(N, D), gain=(N,), bias=(N,), shift=(D,), scale=(D,), in0=(B, D),
                                            in1=(B, D), training=(B, O), out=(B, O), u_add=(B, O)).items()}
    st_arr = {k: np.zeros(s) for k, s in dict(x_f=(B, D), e_f=(B, O), v=(B, N), ref=(B, N), a_f=(B, N), W=(B, O, N),
                                               out_f=(B, O)).items()}
    st = _abi.AdaptState()
    for k, a in st_arr.items():
        setattr(st, k, None if k in state_null else a.ctypes.data)
    g = lambda k: None if k in null else arr[k].ctypes.data
    rc = lib().abrk_adapt_step_batch(dtype, C.byref(p) if params else None, B_, g("enc"), g("gain"), g("bias"),
                                     g("shift"), g("scale"), g("in0"), w0, g("in1") if w1 or "in1" not in null else None,
                                     w1, g("training"), C.byref(st) if state else None, g("out"), g("u_add"), 0, None)
    return rc, lib().abrk_last_error().decode()


EINVAL_CASES = {
    "dtype": dict(dtype=2),
    "neuron type": dict(neuron_type=2),
    "negative batch": dict(B_=-1),
    "no inputs": dict(n_input=0, w0=0),
    "too many inputs": dict(n_input=_abi.ADAPT_MAX_INPUT + 1, w0=_abi.ADAPT_MAX_INPUT + 1),
    "no outputs": dict(n_output=0),
    "too many outputs": dict(n_output=_abi.ADAPT_MAX_OUTPUT + 1),
    "no neurons": dict(n_neurons_total=0),
    "no neurons per ensemble": dict(n_per_ensemble=0),
    "widths do not add up": dict(w0=D - 1, w1=0),
    "widths exceed D": dict(w0=D, w1=1),
    "w1 without in1": dict(w0=D - 1, w1=1, null=("in1",)),
    "dt": dict(dt=0.0),
    "dt nan": dict(dt=float("nan")),
    "tau_rc": dict(tau_rc=0.0),
    "negative tau": dict(tau_input=-1.0),
    "infinite rate": dict(pes_learning_rate=float("inf")),
    "params": dict(params=False),
    "state": dict(state=False),
    **{f"{k} is NULL": dict(null=(k,)) for k in ("enc", "gain", "bias", "shift", "scale", "in0", "training", "out")},
    **{f"state {k} is NULL": dict(state_null=(k,)) for k in ("x_f", "e_f", "v", "ref", "a_f", "W", "out_f")},
}


@pytest.mark.parametrize("what", list(EINVAL_CASES))
def test_einval(what):
    rc, msg = _call(**EINVAL_CASES[what])
    assert rc == -1 and msg, (rc, msg)


def test_an_empty_batch_and_optional_arrays_pass_the_checks():
    # B == 0 returns before the device is touched: what is optional is accepted
    assert _call(B_=0)[0] == 0
    assert _call(B_=0, null=("u_add", "in1"))[0] == 0
    assert _call(B_=0, w0=D - 1, w1=1)[0] == 0
    assert _call(B_=0, neuron_type=_abi.ADAPT_LIF_RATE, state_null=("v", "ref"))[0] == 0


def test_constructor_has_the_references_arguments_then_ours():
    sig = inspect.signature(DynamicsAdaptation.__init__)
    got = [(k, p.default) for k, p in sig.parameters.items() if k != "self"]
    reference = [("n_input", inspect.Parameter.empty), ("n_output", inspect.Parameter.empty), ("n_neurons", 1000),
                 ("n_ensembles", 1), ("seed", None), ("pes_learning_rate", 1e-6), ("intercepts", None),
                 ("weights", None), ("encoders", None), ("spherical", False), ("means", None), ("variances", None),
                 ("tau_input", 0.012), ("tau_training", 0.012), ("tau_output", 0.2), ("dt", 0.001)]
    assert got[:len(reference)] == reference
    ours = dict(got[len(reference):])
    assert list(ours) == ["neuron_type", "max_rates", "dtype", "device", "stream"]
    assert ours["neuron_type"] == "lif" and ours["max_rates"] is None
    p = _abi.make_adapt_params(12, 6)
    assert (p.n_neurons_total, p.n_per_ensemble, p.neuron_type) == (1000, 1000, _abi.ADAPT_LIF)
    assert (p.tau_rc, p.tau_ref, p.dt) == (0.02, 0.002, 0.001)
    assert _abi.make_adapt_params(12, 6, 500, 3).n_neurons_total == 1500


def test_gain_and_bias_of_two_neurons_by_hand():
    # tau_rc = 0.02, tau_ref = 0.002.  Neuron A: intercept 0, max rate 1 / (0.002 + 0.02 ln 2) Hz, for which
    # exp((tau_ref - 1/rate) / tau_rc) = exp(-ln 2) = 1/2, x = 2: gain = (1 - 2) / (0 - 1) = 1, bias = 1 - 0 = 1.
    # Neuron B: intercept 0.5, max rate 1 / (0.002 + 0.02 ln 4): exp(..) = 1/4, x = 4/3: gain = (-1/3) / (-1/2) = 2/3,
    # bias = 1 - (2/3)(1/2) = 2/3.
    rates = [1.0 / (0.002 + 0.02 * np.log(2.0)), 1.0 / (0.002 + 0.02 * np.log(4.0))]
    gain, bias = _abi.lif_gain_bias([0.0, 0.5], rates)
    np.testing.assert_allclose(gain, [1.0, 2.0 / 3.0], rtol=1e-12)
    np.testing.assert_allclose(bias, [1.0, 2.0 / 3.0], rtol=1e-12)
    # the two defining properties: J = 1 at the intercept, the LIF rate at J(1) is the max rate
    J1 = gain + bias
    np.testing.assert_allclose(1.0 / (0.002 + 0.02 * np.log1p(1.0 / (J1 - 1.0))), rates, rtol=1e-12)
    adapt = DynamicsAdaptation(2, 1, n_neurons=2, intercepts=[0.0, 0.5], max_rates=rates, encoders=[[3.0, 4.0], [0.0, -2.0]])
    np.testing.assert_allclose(adapt.gain, gain)
    np.testing.assert_allclose(adapt.bias, bias)
    np.testing.assert_allclose(adapt.encoders[0], [[0.6, 0.8], [0.0, -1.0]])  # unit rows


def test_spherical_is_refused():
    with pytest.raises(NotImplementedError):
        DynamicsAdaptation(4, 2, n_neurons=10, intercepts=np.zeros(10), spherical=True)


def test_unknown_neuron_type_and_widths_are_refused():
    with pytest.raises(ValueError):
        DynamicsAdaptation(4, 2, n_neurons=10, intercepts=np.zeros(10), neuron_type="relu")
    with pytest.raises(ValueError):
        DynamicsAdaptation(4, _abi.ADAPT_MAX_OUTPUT + 1, n_neurons=10, intercepts=np.zeros(10))


class _FakeDeviceArray:
    def __init__(self, a):
        self.a = a

    def numpy(self, stream=None):
        return self.a


def test_a_changed_batch_raises_and_get_weights_shapes(monkeypatch):
    adapt = DynamicsAdaptation(4, 2, n_neurons=10, n_ensembles=3, intercepts=np.zeros(30))
    with pytest.raises(RuntimeError):
        adapt.get_weights()  # nothing allocated yet

    def allocate(self, B):  # the device allocation of the first call, without a device
        self.B = B
        self.state = {"W": _FakeDeviceArray(np.arange(B * 2 * 30, dtype=float).reshape(B, 2, 30))}

    monkeypatch.setattr(DynamicsAdaptation, "_allocate", allocate)
    adapt._rows(5)
    adapt._rows(5)
    with pytest.raises(ValueError, match="5 rows"):
        adapt._rows(6)
    with pytest.raises(ValueError, match="5 rows"):
        adapt.generate(np.zeros(4), np.zeros(2))  # a single state after a batch of 5
    W = adapt.get_weights()
    assert len(W) == 3 and all(w.shape == (5, 2, 10) for w in W)
    np.testing.assert_array_equal(W[1][2, 1], np.arange(10) + 2 * 60 + 30 + 10)


def test_means_and_variances_fill_each_other_in_and_scale_inputs():
    adapt = DynamicsAdaptation(2, 1, n_neurons=4, intercepts=np.zeros(4), means=np.array([1.0, 2.0]))
    np.testing.assert_array_equal(adapt.variances, [1.0, 1.0])
    adapt = DynamicsAdaptation(2, 1, n_neurons=4, intercepts=np.zeros(4), variances=np.array([2.0, 4.0]))
    np.testing.assert_array_equal(adapt.means, [0.0, 0.0])
    np.testing.assert_allclose(adapt.scale_inputs([[2.0, 2.0]]), [[1.0, 0.5]])


def test_default_intercepts_follow_the_references_distribution():
    pytest.importorskip("scipy")
    adapt = DynamicsAdaptation(12, 6, n_neurons=200, n_ensembles=2, seed=3)
    assert adapt.intercepts.shape == (2, 200) and adapt.max_rates.shape == (2, 200)
    # CosineSimilarity(14).ppf(1 - p), p triangular on 0.35..0.55: p = 0.5 is intercept 0, so the intercepts straddle it
    # and stay small - |ppf| <= ppf(0.65) of the 14-dimensional distribution, about 0.11
    assert adapt.intercepts.min() < 0 < adapt.intercepts.max() and np.abs(adapt.intercepts).max() < 0.15
    assert 200 <= adapt.max_rates.min() and adapt.max_rates.max() <= 400
    again = DynamicsAdaptation(12, 6, n_neurons=200, n_ensembles=2, seed=3)
    np.testing.assert_array_equal(adapt.encoders, again.encoders)
    np.testing.assert_allclose(np.linalg.norm(adapt.encoders, axis=-1), 1.0)
