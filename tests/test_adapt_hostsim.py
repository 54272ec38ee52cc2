"""The adaptive signal's row program, built for the host (tests/hostsim_adapt), against its NumPy statement
(tests/adapt_ref.py): 40 ticks in fp64, both neuron types, three shapes (tests/adapt_cases.py).  Bound: 1e-9 of the
case's largest |value|, for every tick's output and for the final weights - the bar of the path planner and IK tests.
The spiking decision v > 1 is a comparison: the bound presumes that no decision of the reference was closer to a tie
than 1e-9, and the test asserts that it was not.

The path cases (adapt_cases.PATH_CASES) put shift and scale, the input in two arrays, the zero time constants, other
steps and neuron constants, several ensembles and nonzero initial weights under the same bound, for every tick's output
and all seven state arrays (adapt_cases.state_errors)."""
import numpy as np
import pytest

from tests import adapt_cases, hostsim_adapt


@pytest.mark.parametrize("neuron_type", ["lif", "lif_rate"])
@pytest.mark.parametrize("index", range(len(adapt_cases.PARITY_SHAPES)))
def test_host_build_matches_the_numpy_reference(index, neuron_type):
    case, outs, state, _near, margin = adapt_cases.reference("parity", index, neuron_type)
    if neuron_type == "lif":
        print(f"smallest |v - 1| of the reference: {margin.min():.3e}")
        assert margin.min() >= 1e-9
    host = hostsim_adapt.HostAdapt(case.enc, case.gain, case.bias, case.B, case.O, case.n_per, neuron_type, **case.kw)
    got = case.run(host)
    assert np.abs(outs).max() > 0 and np.abs(state["W"]).max() > 0
    eo = np.abs(got - outs).max() / np.abs(outs).max()
    ew = np.abs(host.state()["W"] - state["W"]).max() / np.abs(state["W"]).max()
    print(f"{adapt_cases.PARITY_SHAPES[index]} {neuron_type}: out {eo:.2e}, W {ew:.2e}")
    assert eo <= 1e-9 and ew <= 1e-9, (eo, ew)
    if neuron_type == "lif":  # the voltages and refractory times themselves
        for k in ("v", "ref", "a_f"):
            assert np.abs(host.state()[k] - state[k]).max() <= 1e-9 * max(np.abs(state[k]).max(), 1.0), k


@pytest.mark.parametrize("neuron_type", ["lif", "lif_rate"])
@pytest.mark.parametrize("name", list(adapt_cases.PATH_CASES))
def test_host_build_matches_the_numpy_reference_on_the_path_cases(name, neuron_type):
    case, outs, state, _near, margin = adapt_cases.reference("path", name, neuron_type)
    if neuron_type == "lif":
        print(f"smallest |v - 1| of the reference: {margin.min():.3e}")
        assert margin.min() >= 1e-9
    host = hostsim_adapt.HostAdapt(case.enc, case.gain, case.bias, case.B, case.O, case.n_per, neuron_type,
                                   split=case.split, **case.tables, **case.kw)
    got = case.run(host)
    eo = adapt_cases.out_error(outs, got)
    errs = adapt_cases.state_errors(state, host.state())
    print(f"{name} {neuron_type}: out {eo:.2e}, " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert set(errs) == set(adapt_cases.STATE)
    assert eo <= 1e-9, eo
    assert max(errs.values()) <= 1e-9, errs
