"""The adaptive signal on the GPU (abrk_adapt_step_batch / engine.adapt_step / DynamicsAdaptation) against its NumPy
statement (tests/adapt_ref.py), on the cases of tests/adapt_cases.py.

  a  fp64, both neuron types, three shapes, 40 ticks: every tick's output and the final weights within 1e-9 of the case's
     largest |value| - on condition that no spiking decision of the reference was closer to a tie than 1e-9 (asserted)
  b  fp32 lif_rate: within 1e-4, the package's fp32 bar
  c  fp32 lif: a row in which the fp64 reference has a neuron-step with |v - 1| < 1e-4 may decide a spike differently in
     fp32 (the voltage error with gains <= ~50 is below 1e-5) and is left out; the others meet 1e-4; at most a quarter of
     the rows may be left out
  d  a row's bits do not depend on the batch: rows 0..69 in one call of 70 and in calls of 1, 6 and 63
  e  a recorded plan replayed by launch_graph(20) equals 20 single calls bit for bit; u_add accumulates into the u the
     recorded law wrote just before
  f  the closed loop of examples/adaptive_ur5_headless.py tracks better with the adaptive signal than without

On the path cases (adapt_cases.PATH_CASES: the kernel paths and parameters that the three shapes do not reach), with
all seven state arrays compared by adapt_cases.state_errors:
  g  fp64, both neuron types, at 1e-9 (on the condition of a); fp32 lif_rate at 1e-4
  h  fp32 lif neuron by neuron: neurons are independent of one another in everything but `out`, so v, ref, a_f and
     W[:, :, i] of every neuron without a step within 1e-4 of the threshold in the reference meet 1e-4; at most 2 % of a
     row's neurons may be left out (intercepts within +-0.2: gains <= 49.4)
  i  every per-neuron array one element into a larger buffer (V = 1 on arrays whose length would allow 16 bytes per
     lane) meets the bars of g; the encoder table alone one element in gives the bits of the aligned run
  j  guard rows of 0xFF bytes around every array the tick writes stay 0xFF, and the results are those on plain arrays
  k  the NumPy form of engine.adapt_step gives the bits of the DeviceArray form; u_add accumulates over the ticks
  l  DynamicsAdaptation(means=, variances=, weights=) with two ensembles against the reference"""
import importlib.util
import os

import numpy as np
import pytest

import abr_control_amd as a
from abr_control_amd import _abi, engine
from tests import adapt_cases

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("x_f", "e_f", "v", "ref", "a_f", "W", "out_f")


def _ff_filled(shape, dtype):
    """a DeviceArray of all-ones bytes (NaN in both types), as _nan_filled of tests/test_channel_gpu.py"""
    arr = a.DeviceArray(shape, dtype)
    engine.check(engine.lib().abrk_memset(0, arr.ptr, 0xFF, arr.nbytes, None))
    return arr


def _one_element_in(shape, dtype):
    """a DeviceArray of `shape` that starts one element into a larger buffer: rows 1.. of a flat array, given the shape
    of the call (8 or 4 bytes past a 16-byte boundary)"""
    n = int(np.prod(shape))
    view = a.DeviceArray((n + 1,), dtype).rows(1, n + 1)
    view.shape = tuple(shape)
    assert view.ptr % 16 == np.dtype(dtype).itemsize
    return view


PER_NEURON = ("gain", "bias", "a_f", "v", "ref", "W")


class GpuAdapt:
    """rows `rows` of a case stepped by engine.adapt_step, with tick() of adapt_ref.AdaptRef.  The case's shift, scale
    and W0 are applied, and its input goes in as in0 and in1 where the case has a split.
      form: "device" (DeviceArrays) | "numpy" (every argument a NumPy array, staged by the library)
      u_add: [B, O] - u_add of every tick, starting from these values and never zeroed
      offset: names among enc, gain, bias, a_f, v, ref, W - allocated one element into a larger buffer
      guard: every array the tick writes (the state, out, u_add) is rows 1..B of a buffer of B + 2 rows of 0xFF bytes
      v_ref: False leaves v and ref out of the state dict (lif_rate)"""

    def __init__(self, case, neuron_type, dtype, rows=slice(None), form="device", u_add=None, offset=(), guard=False,
                 v_ref=True):
        assert form in ("device", "numpy") and (form == "device" or not (offset or guard)) and not (offset and guard)
        self.dtype = np.dtype(dtype)
        self.form = form
        self.B = B = len(range(case.B)[rows])
        self.split = case.split
        self.params = _abi.make_adapt_params(case.D, case.O, case.n_per, case.n_ens, neuron_type, **case.kw)
        host = lambda x: np.ascontiguousarray(x, dtype=self.dtype)
        tables = {"enc": case.enc, "gain": case.gain, "bias": case.bias,
                  "shift": np.zeros(case.D) if case.shift is None else case.shift,
                  "scale": np.ones(case.D) if case.scale is None else case.scale}
        shapes = dict(engine.adapt_state_shapes(self.params, B))
        init = {k: np.zeros(sh) for k, sh in shapes.items()}
        if case.W0 is not None:
            init["W"] = np.broadcast_to(case.W0, shapes["W"])
        if not v_ref:
            del init["v"], init["ref"]
        init["out"] = np.zeros((B, case.O))
        if u_add is not None:
            init["u_add"] = np.asarray(u_add)[rows]
        self.guards = {}
        if form == "numpy":
            self.tables = [host(x) for x in tables.values()]
            arrs = {k: host(x).copy() for k, x in init.items()}
        else:
            self.tables = [(_one_element_in(np.shape(x), self.dtype).copy_from_numpy(host(x)) if k in offset else
                            a.DeviceArray.from_numpy(host(x))) for k, x in tables.items()]
            arrs = {}
            for k, x in init.items():
                if guard:
                    self.guards[k] = _ff_filled((B + 2,) + x.shape[1:], self.dtype)
                    arrs[k] = self.guards[k].rows(1, B + 1)
                elif k in offset:
                    arrs[k] = _one_element_in(x.shape, self.dtype)
                else:
                    arrs[k] = a.DeviceArray(x.shape, self.dtype)
                arrs[k].copy_from_numpy(host(x))
            w0 = case.D if self.split is None else self.split[0]
            self.x0, self.t = a.DeviceArray((B, w0), self.dtype), a.DeviceArray((B, case.O), self.dtype)
            self.x1 = None if self.split is None else a.DeviceArray((B, case.D - w0), self.dtype)
        self.out, self.u_add = arrs.pop("out"), arrs.pop("u_add", None)
        self.st = arrs

    def tick(self, x, training):
        x, training = np.asarray(x, dtype=self.dtype), np.asarray(training, dtype=self.dtype)
        x0, x1 = (x, None) if self.split is None else (x[:, :self.split[0]], x[:, self.split[0]:])
        if self.form == "device":
            x0, training = self.x0.copy_from_numpy(x0), self.t.copy_from_numpy(training)
            x1 = None if x1 is None else self.x1.copy_from_numpy(x1)
        out = engine.adapt_step(self.params, *self.tables, x0, training, self.st, in1=x1, out=self.out, u_add=self.u_add,
                                dtype=self.dtype)
        assert out is self.out
        return self.out.numpy() if self.form == "device" else self.out.copy()

    def state(self):
        return {k: (v.numpy() if self.form == "device" else v.copy()) for k, v in self.st.items()}

    def u_added(self):
        return self.u_add.numpy() if self.form == "device" else self.u_add.copy()

    def touched_guards(self):
        """the names of the arrays whose spare row before or after no longer holds 0xFF bytes"""
        bad = []
        for k, buf in self.guards.items():
            rows = buf.numpy().view(np.uint8).reshape(self.B + 2, -1)
            if not ((rows[0] == 0xFF).all() and (rows[-1] == 0xFF).all()):
                bad.append(k)
        return bad


def _fmt(errs):
    return ", ".join(f"{k} {e:.2e}" for k, e in errs.items())


def _errors(case, outs, state, got, got_state, rows=slice(None)):
    eo = np.abs(got[:, rows] - outs[:, rows]).max() / np.abs(outs[:, rows]).max()
    ew = np.abs(got_state["W"][rows] - state["W"][rows]).max() / np.abs(state["W"][rows]).max()
    return eo, ew


@pytest.mark.parametrize("neuron_type", ["lif", "lif_rate"])
@pytest.mark.parametrize("index", range(len(adapt_cases.PARITY_SHAPES)))
def test_fp64_matches_the_numpy_reference(index, neuron_type):
    case, outs, state, _near, margin = adapt_cases.reference("parity", index, neuron_type)
    if neuron_type == "lif":
        assert margin.min() >= 1e-9
    g = GpuAdapt(case, neuron_type, np.float64)
    got = case.run(g)
    eo, ew = _errors(case, outs, state, got, g.state())
    print(f"{adapt_cases.PARITY_SHAPES[index]} {neuron_type} fp64: out {eo:.2e}, W {ew:.2e}")
    assert eo <= 1e-9 and ew <= 1e-9, (eo, ew)
    errs = adapt_cases.state_errors(state, g.state())
    print("state: " + _fmt(errs))
    assert set(errs) == set(STATE) and max(errs.values()) <= 1e-9, errs


@pytest.mark.parametrize("index", range(len(adapt_cases.PARITY_SHAPES)))
def test_fp32_rates_match_the_numpy_reference(index):
    case, outs, state, _near, _margin = adapt_cases.reference("parity", index, "lif_rate")
    g = GpuAdapt(case, "lif_rate", np.float32)
    got = case.run(g)
    eo, ew = _errors(case, outs, state, got, g.state())
    print(f"{adapt_cases.PARITY_SHAPES[index]} lif_rate fp32: out {eo:.2e}, W {ew:.2e}")
    assert eo <= 1e-4 and ew <= 1e-4, (eo, ew)


@pytest.mark.parametrize("index", range(len(adapt_cases.F32_LIF_CASES)))
def test_fp32_spikes_match_the_numpy_reference_away_from_the_threshold(index):
    case, outs, state, near, _margin = adapt_cases.reference("f32lif", index, "lif")
    keep = near == 0
    print(f"{adapt_cases.F32_LIF_CASES[index]}: {np.sum(~keep)} of {case.B} rows left out, gains up to {case.gain.max():.1f}")
    assert np.sum(~keep) <= case.B // 4
    g = GpuAdapt(case, "lif", np.float32)
    got = case.run(g)
    eo, ew = _errors(case, outs, state, got, g.state(), rows=keep)
    print(f"lif fp32: out {eo:.2e}, W {ew:.2e}")
    assert eo <= 1e-4 and ew <= 1e-4, (eo, ew)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("neuron_type", ["lif", "lif_rate"])
@pytest.mark.parametrize("N", [257, 260])  # element-wise, and 16 bytes per lane in both types
def test_a_rows_bits_do_not_depend_on_the_batch(N, neuron_type, dtype):
    case = adapt_cases.Case((70, N, 12, 6, 1), 10, 0.9, 300 + N)
    whole = GpuAdapt(case, neuron_type, dtype)
    outs = case.run(whole)
    st = whole.state()
    assert np.abs(outs).max() > 0
    for rows in (slice(0, 1), slice(1, 7), slice(7, 70)):
        part = GpuAdapt(case, neuron_type, dtype, rows)
        assert part.B == rows.stop - rows.start
        got = case.run(part, rows)
        assert np.array_equal(got, outs[:, rows]), rows
        pst = part.state()
        for k in STATE:
            assert np.array_equal(pst[k], st[k][rows]), (k, rows)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_plan_replay_equals_single_calls(dtype):
    from abr_control_amd.arms import ur5

    B, n, N, K = 70, 6, 260, 20
    rc = ur5.Config()
    rng = np.random.RandomState(5)
    q0, dq0 = rng.uniform(-1, 1, (B, n)), rng.uniform(-0.5, 0.5, (B, n))
    target = rng.uniform(-0.5, 0.5, (B, 6))
    case = adapt_cases.Case((B, N, 2 * n, n, 1), 1, 0.5, 77)
    law = _abi.make_osc_params(n, kp=50, use_C=True, use_g=True)
    params = _abi.make_adapt_params(2 * n, n, N, 1, "lif", dt=0.001, pes_learning_rate=1e-4)
    stream = a.Stream(0)
    dev = lambda x: a.DeviceArray.from_numpy(np.ascontiguousarray(x, dtype=dtype))
    tables = [dev(x) for x in (case.enc, case.gain, case.bias, np.zeros(2 * n), np.ones(2 * n))]
    q, dq, tgt = dev(q0), dev(dq0), dev(target)

    def fresh():
        st = {k: a.DeviceArray(sh, dtype).zero_(stream) for k, sh in engine.adapt_state_shapes(params, B).items()}
        return st, a.DeviceArray((B, n), dtype).zero_(stream), a.DeviceArray((B, n), dtype).zero_(stream)

    def tick(st, u, ts):
        engine.osc_generate(rc.arm_id, n, law, q, dq, tgt, u=u, training_signal=ts, dtype=dtype, stream=stream)
        return engine.adapt_step(params, *tables, q, ts, st, in1=dq, u_add=u, dtype=dtype, stream=stream)

    st1, u1, ts1 = fresh()
    for _ in range(K):
        out1 = tick(st1, u1, ts1)
    st2, u2, ts2 = fresh()
    with engine.Plan(device=0, stream=stream) as plan:
        out2 = tick(st2, u2, ts2)
    plan.launch_graph(K)
    law_u = engine.osc_generate(rc.arm_id, n, law, q, dq, tgt, dtype=dtype, stream=stream).numpy(stream)
    o1, o2 = out1.numpy(stream), out2.numpy(stream)
    assert np.abs(o1).max() > 0 and np.array_equal(o1, o2)
    for k in STATE:
        assert np.array_equal(st1[k].numpy(stream), st2[k].numpy(stream)), k
    # u is what the law wrote in this tick plus this tick's adaptive signal: nothing of earlier ticks is left in it
    assert np.array_equal(u2.numpy(stream), law_u + o2) and np.array_equal(u1.numpy(stream), u2.numpy(stream))


def test_generate_takes_one_state_or_a_batch_and_keeps_its_batch():
    from abr_control_amd.controllers.signals import DynamicsAdaptation

    kw = dict(n_neurons=50, n_ensembles=2, intercepts=np.linspace(-0.5, 0.5, 100), seed=1, pes_learning_rate=1e-3)
    one = DynamicsAdaptation(4, 2, **kw)
    many = DynamicsAdaptation(4, 2, **kw)
    x, t = np.array([0.3, -0.2, 0.5, 0.1]), np.array([1.0, -2.0])
    for _ in range(40):  # (spiking neurons start at v = 0: their first spikes, and with them the first output, take a few ms)
        o1 = one.generate(x, t)
        o3 = many.generate(np.tile(x, (3, 1)), np.tile(t, (3, 1)))
    assert o1.shape == (2,) and o3.shape == (3, 2) and np.abs(o1).max() > 0
    assert np.array_equal(o3, np.tile(o1, (3, 1)))
    W = many.get_weights()
    assert len(W) == 2 and W[0].shape == (3, 2, 50)
    with pytest.raises(ValueError):
        many.generate(x, t)
    many.reset()
    assert np.abs(many.get_weights()[0]).max() == 0
    assert np.array_equal(many.generate(np.tile(x, (3, 1)), np.tile(t, (3, 1)))[0], one_first(kw, x, t))


def one_first(kw, x, t):
    from abr_control_amd.controllers.signals import DynamicsAdaptation

    return DynamicsAdaptation(4, 2, **kw).generate(x, t)


# ------------------------------------------------------------------------------------------------- the path cases
PATHS = list(adapt_cases.PATH_CASES)
F64, F32 = np.float64, np.float32
# (dtype, neuron_type) whose results are held to the reference over whole rows, and the bar
REFERENCE_BARS = {(F64, "lif"): 1e-9, (F64, "lif_rate"): 1e-9, (F32, "lif_rate"): 1e-4}


def _check_against_reference(label, name, neuron_type, dtype, **how):
    """runs a path case on the GPU and holds every tick's output and all seven state arrays to the reference at the
    bar of (dtype, neuron_type)"""
    bar = REFERENCE_BARS[(dtype, neuron_type)]
    case, outs, state, _near, margin = adapt_cases.reference("path", name, neuron_type)
    if neuron_type == "lif":
        assert margin.min() >= 1e-9
    g = GpuAdapt(case, neuron_type, dtype, **how)
    got = case.run(g)
    eo = adapt_cases.out_error(outs, got)
    print(f"{label} {name} {neuron_type} {np.dtype(dtype).name}: out {eo:.2e}")
    assert eo <= bar, eo
    errs = adapt_cases.state_errors(state, g.state())
    print("state: " + _fmt(errs))
    assert set(errs) == set(STATE) and max(errs.values()) <= bar, errs


def _bits_equal(one, other, outs_one, outs_other):
    assert np.abs(outs_one).max() > 0 and outs_one.tobytes() == outs_other.tobytes()
    s1, s2 = one.state(), other.state()
    for k in s1.keys() & s2.keys():
        assert s1[k].tobytes() == s2[k].tobytes(), k
    return s1.keys() & s2.keys()


@pytest.mark.parametrize("neuron_type", ["lif", "lif_rate"])
@pytest.mark.parametrize("name", PATHS)
def test_fp64_matches_the_numpy_reference_on_the_path_cases(name, neuron_type):
    _check_against_reference("path", name, neuron_type, F64)


@pytest.mark.parametrize("name", PATHS)
def test_fp32_rates_match_the_numpy_reference_on_the_path_cases(name):
    _check_against_reference("path", name, "lif_rate", F32)


def _gap_history(case, b, i):
    """|v - 1| of neuron i of row b at every tick's threshold decision, from the reference (the neuron alone: its voltage
    depends on nothing but the row's input)"""
    from tests import adapt_ref

    one = adapt_ref.AdaptRef(case.enc[i:i + 1], case.gain[i:i + 1], case.bias[i:i + 1], 1, case.O, 1, "lif",
                             shift=case.shift, scale=case.scale, **case.kw)
    hist = []
    for k in range(case.ticks):
        one.margin[:] = np.inf
        one.tick(case.x[k, b:b + 1], case.training[k, b:b + 1])
        hist.append(one.margin[0])
    return hist


@pytest.mark.parametrize("index", range(len(adapt_cases.F32_LIF_NEURON_SHAPES)))
def test_fp32_spikes_match_the_numpy_reference_neuron_by_neuron(index):
    """Shapes of three passes (2052) and two (1028) with 16 bytes per lane, two ensembles, O = 16.  Intercepts within
    +-0.2 and rates <= 400 Hz keep every gain <= 49.4 (the closed form of lif_gain_bias at 400 Hz and 0.2), the regime of
    the 1e-4 band (c above)."""
    case, _outs, ref = adapt_cases.reference_model("f32lif_n", index, "lif")
    keep = ~ref.near_n
    left_out = ref.near_n.mean(axis=1)
    print(f"{adapt_cases.F32_LIF_NEURON_SHAPES[index]}: {ref.near_n.sum()} neurons left out, at most "
          f"{100 * left_out.max():.2f} % of a row; gains up to {case.gain.max():.1f}")
    assert case.gain.max() <= 49.4
    assert left_out.max() <= 0.02
    g = GpuAdapt(case, "lif", F32)
    case.run(g)
    got = g.state()
    errs = adapt_cases.state_errors(ref.state(), {k: got[k] for k in ("x_f", "e_f", "v", "ref", "a_f", "W")},
                                    neurons=keep)
    print("lif fp32 by neuron: " + _fmt(errs))
    if max(errs.values()) > 1e-4:  # the kept neuron furthest off in a_f (a spike more or less shows there), and how
        # close its decisions came to a tie in the reference
        diff = np.where(keep, np.abs(got["a_f"] - ref.a_f), 0.0)
        b, i = np.unravel_index(np.argmax(diff), diff.shape)
        hist = _gap_history(case, b, i)
        print(f"row {b} neuron {i}: a_f {got['a_f'][b, i]} against {ref.a_f[b, i]}, gain {case.gain[i]:.2f}; "
              f"|v - 1| of the reference per tick: " + " ".join(f"{h:.2e}" for h in hist))
    assert max(errs.values()) <= 1e-4, errs


@pytest.mark.parametrize("name, dtype, neuron_type", [
    ("odd_all", F64, "lif"), ("odd_all", F64, "lif_rate"), ("odd_all", F32, "lif_rate"),
    ("passes64", F64, "lif"), ("passes64", F64, "lif_rate")])
def test_unaligned_per_neuron_arrays_take_one_element_per_lane(name, dtype, neuron_type):
    """N % (16 / sizeof(T)) == 0, so only the addresses send these calls down V = 1"""
    case = adapt_cases.reference("path", name, neuron_type)[0]
    assert case.N % (16 // np.dtype(dtype).itemsize) == 0
    _check_against_reference("one element in", name, neuron_type, dtype, offset=PER_NEURON)


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("neuron_type", ["lif", "lif_rate"])
@pytest.mark.parametrize("name", ["passes64", "max_in"])
def test_an_unaligned_encoder_table_gives_the_same_bits(name, neuron_type, dtype):
    """D % (16 / sizeof(T)) == 0: the encoder table's address alone decides between dot_vec and adapt_dot, which form
    the same products in the same order (abrk_adapt.hip)"""
    case = adapt_cases.reference("path", name, neuron_type)[0]
    assert case.D % (16 // np.dtype(dtype).itemsize) == 0
    aligned, unaligned = GpuAdapt(case, neuron_type, dtype), GpuAdapt(case, neuron_type, dtype, offset=("enc",))
    assert len(_bits_equal(aligned, unaligned, case.run(aligned), case.run(unaligned))) == 7


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("neuron_type", ["lif", "lif_rate"])
@pytest.mark.parametrize("name", ["max_out", "odd_all", "passes32"])
def test_nothing_is_written_outside_the_rows(name, neuron_type, dtype):
    """even N: the views of rows 1..B are as aligned as the buffers, so odd_all in fp32 and passes32 store 16 bytes per
    lane next to the guard rows"""
    case = adapt_cases.reference("path", name, neuron_type)[0]
    zeros = np.zeros((case.B, case.O))
    plain, guarded = GpuAdapt(case, neuron_type, dtype, u_add=zeros), GpuAdapt(case, neuron_type, dtype, u_add=zeros,
                                                                                guard=True)
    assert set(guarded.guards) == set(STATE) | {"out", "u_add"}
    assert guarded.touched_guards() == []
    assert len(_bits_equal(plain, guarded, case.run(plain, ticks=5), case.run(guarded, ticks=5))) == 7
    assert plain.u_added().tobytes() == guarded.u_added().tobytes()
    assert guarded.touched_guards() == []


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("neuron_type", ["lif", "lif_rate"])
@pytest.mark.parametrize("name", ["odd_all", "passes64"])
def test_numpy_arguments_give_the_bits_of_device_arrays_and_u_add_accumulates(name, neuron_type, dtype):
    K = 5
    case, outs, _state, _near, _margin = adapt_cases.reference("path", name, neuron_type)
    fill = np.random.RandomState(11).uniform(-1.0, 1.0, (case.B, case.O)).astype(dtype)
    # lif_rate: the NumPy call's state has no v and ref
    dev = GpuAdapt(case, neuron_type, dtype, u_add=fill)
    host = GpuAdapt(case, neuron_type, dtype, u_add=fill, form="numpy", v_ref=neuron_type == "lif")
    od, oh = case.run(dev, ticks=K), case.run(host, ticks=K)
    assert len(_bits_equal(dev, host, od, oh)) == (7 if neuron_type == "lif" else 5)
    u = dev.u_added()
    assert u.tobytes() == host.u_added().tobytes()
    # u_add is never zeroed: the fill plus every tick's output, added in the call's arithmetic
    own = fill.copy()
    for k in range(K):
        own += od[k]
    assert u.tobytes() == own.tobytes()
    if (dtype, neuron_type) in REFERENCE_BARS:
        want = fill.astype(np.float64) + outs[:K].sum(axis=0)
        err = np.abs(u - want).max() / max(np.abs(want).max(), 1.0)
        print(f"u_add {name} {neuron_type} {np.dtype(dtype).name}: {err:.2e}")
        assert err <= REFERENCE_BARS[(dtype, neuron_type)], err


@pytest.mark.parametrize("neuron_type", ["lif", "lif_rate"])
def test_dynamics_adaptation_with_means_variances_and_weights(neuron_type):
    from abr_control_amd.controllers.signals import DynamicsAdaptation
    from tests import adapt_ref

    B, n, D, O, seed = 3, 65, 5, 3, 430
    enc, intercepts, max_rates = adapt_ref.population_parts(2 * n, D, seed)
    rng = np.random.RandomState(seed + 7)
    means, variances = rng.uniform(-0.3, 0.3, D), rng.uniform(0.5, 1.5, D)
    weights = rng.uniform(-1e-3, 1e-3, (2, O, n))
    case = adapt_cases.Case((B, 2 * n, D, O, 2), 40, 0.9, seed, shift=means, scale=1.0 / variances,
                            W0=np.concatenate([weights[0], weights[1]], axis=1))
    assert np.array_equal(case.enc, enc)
    ref = adapt_ref.AdaptRef(case.enc, case.gain, case.bias, B, O, n, neuron_type, **case.tables, **case.kw)
    outs = case.run(ref)
    if neuron_type == "lif":
        assert ref.margin.min() >= 1e-9
    adapt = DynamicsAdaptation(D, O, n_neurons=n, n_ensembles=2, pes_learning_rate=adapt_cases.LEARNING_RATE,
                               intercepts=intercepts, max_rates=max_rates, encoders=enc, weights=weights, means=means,
                               variances=variances, neuron_type=neuron_type)
    got = np.stack([adapt.generate(case.x[k], case.training[k]) for k in range(case.ticks)])
    eo = adapt_cases.out_error(outs, got)
    errs = adapt_cases.state_errors(ref.state(), {k: v.numpy() for k, v in adapt.state.items()})
    print(f"DynamicsAdaptation {neuron_type}: out {eo:.2e}, " + _fmt(errs))
    assert eo <= 1e-9 and set(errs) == set(STATE) and max(errs.values()) <= 1e-9, (eo, errs)
    W = adapt.get_weights()
    assert len(W) == 2
    top = np.abs(ref.W).max()
    for e in range(2):
        assert W[e].shape == (B, O, n)
        assert np.abs(W[e] - ref.W[:, :, e * n:(e + 1) * n]).max() <= 1e-9 * top, e


CLOSED_LOOP_TICKS = 3000
# The same loop on the CPU - the host builds of the law (tests/hostsim), the plant (tests/hostsim_plant) and the adaptive
# signal (tests/hostsim_adapt), fp64, 64 arms, 3000 ticks, pes_learning_rate = 2e-4 (the example's default; 2e-3 drives some
# arms unstable, 5e-5 has not converged after 3000 ticks) - gave, over the last 500 ticks and averaged over the arms:
HOST_ERR_RMS_PLAIN, HOST_ERR_RMS_ADAPTIVE = 46.423e-3, 0.39611e-3  # m
CLOSED_LOOP_RATIO = 0.5 * HOST_ERR_RMS_PLAIN / HOST_ERR_RMS_ADAPTIVE  # half of 117.2


def test_closed_loop_tracks_better_with_the_adaptive_signal():
    """UR5, 64 arms, lif_rate, the loop of examples/adaptive_ur5_headless.py - { OSC.generate(training_signal); adapt.step;
    plant step with effects and a constant 15 N wrench from tick 0; record } replayed 3000 times: on every arm the
    recorder's err_rms over the last 500 ticks is below that of the same loop without the adaptive signal, and the ratio
    of the two (batch means) is at least half of what the host builds give: 46.423 mm without, 0.396 mm with, ratio
    117.2 (the smallest ratio of a single arm on the host: 5.0)."""
    spec = importlib.util.spec_from_file_location("adaptive_ur5_headless",
                                                  os.path.join(REPO, "examples", "adaptive_ur5_headless.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    plain = mod.run(False, 64, CLOSED_LOOP_TICKS)["err_rms"]
    adaptive = mod.run(True, 64, CLOSED_LOOP_TICKS)["err_rms"]
    ratio = plain / adaptive
    print(f"err_rms over the last 500 ticks: without {plain.mean() * 1e3:.3f} mm, with {adaptive.mean() * 1e3:.3f} mm; "
          f"ratio of the means {plain.mean() / adaptive.mean():.2f}, smallest over the arms {ratio.min():.2f}")
    assert (adaptive < plain).all()
    assert plain.mean() / adaptive.mean() >= CLOSED_LOOP_RATIO
