"""The measurement channel on the GPU (abrk_channel_step_batch / sensing.channel_step / SignalChannel / JointSensor)
against its NumPy statement (tests/channel_ref.py).

  a  8 ticks against the reference: B in {1, 63, 64, 65, 1000}, (w0, w1) in {(1,0), (6,6), (7,0), (16,0), (9,7)}, delay in
     {0, 1, 3}, with and without dy, fp64 and fp32.  Two channels per shape.  "mixed": column c has noise alone (c % 3 == 0),
     bias and quantisation (c % 3 == 1) or bias alone (c % 3 == 2) - the noisy columns within 256 eps64 sigma (the bound of
     tests/test_channel_hostsim.py; inputs and sigma are of order 1, so the last rounding of v stays inside it), plus
     eps32 |v| in fp32 for the final rounding; the others bit for bit.  "encoder": noise and quantisation on every column -
     bit for bit, on condition that no v / resolution of the reference is within 1e-9 of a half-integer (asserted first).
     dy: within 1e-12 (fp64) / 1e-5 (fp32) of the largest |g|.
  b  the transparent channel is the identity bit for bit; with every sigma zero the seed changes nothing
  c  a row's bits do not depend on the batch: rows 300..363 of a 1000-row call against a 64-row call with row_offset 300;
     the arrays may be unaligned row views
  d  launch_graph(8) of a recorded apply() equals 8 single launches bit for bit - outputs, ring, prev, d_f, counter
  e  the statistics of tests/test_channel_hostsim.py on the device's own 393 216 normals
  f  a closed UR5 loop, 64 arms, 50 ticks: with a transparent JointSensor and SignalChannel in the plan the recorded q is
     bit for bit that of the plan without them; with delay = 2 on the sensor q_meas of tick t is the q of tick t - 2"""
import functools

import numpy as np
import pytest

import abr_control_amd as a
from abr_control_amd import _abi, engine, sensing
from tests import channel_ref

pytestmark = pytest.mark.gpu

EPS64, EPS32 = float(np.finfo(np.float64).eps), float(np.finfo(np.float32).eps)
K, BMAX, WMAX = 8, 1000, 16
BATCHES = (1, 63, 64, 65, 1000)
SPLITS = ((1, 0), (6, 6), (7, 0), (16, 0), (9, 7))
SEED = 424242
DT, TAU = 0.001, 0.005
ENCODER = 2 * np.pi / 2 ** 14


@functools.lru_cache(maxsize=None)
def _inputs():
    """xs [K, BMAX, WMAX] in (-1, 1), shared by every case and never written"""
    xs = np.random.RandomState(7).uniform(-1, 1, (K, BMAX, WMAX))
    xs.setflags(write=False)
    return xs


@functools.lru_cache(maxsize=None)
def _normals(seed):
    """n [BMAX, K, WMAX] of rows 0.., ticks 0..K-1: every smaller shape is a corner of it"""
    n = channel_ref.normal_block(seed, np.arange(BMAX), np.arange(K), np.arange(WMAX))
    n.setflags(write=False)
    return n


def _columns(kind, W):
    c = np.arange(W)
    if kind == "mixed":
        return dict(sigma=np.where(c % 3 == 0, 0.5, 0.0), bias=np.where(c % 3 == 0, 0.0, 0.01 * (c + 1)),
                    resolution=np.where(c % 3 == 1, 1e-3, 0.0))
    return dict(sigma=np.full(W, 0.02), bias=np.zeros(W), resolution=np.full(W, ENCODER))


def _nan_filled(shape, dtype):
    """a DeviceArray of all-ones bytes (NaN in both types): what the tick reads before it has written shows"""
    arr = a.DeviceArray(shape, dtype)
    engine.check(engine.lib().abrk_memset(0, arr.ptr, 0xFF, arr.nbytes, None))
    return arr


class GpuChannel:
    """B rows stepped by sensing.channel_step on DeviceArrays, with tick() of channel_ref.ChannelRef"""

    def __init__(self, w0, w1, B, dtype, delay=0, difference=False, tau_diff=0.0, seed=0, row_offset=0, **cols):
        self.w0, self.w1, self.B, self.dtype, self.difference = w0, w1, B, np.dtype(dtype), difference
        W = w0 + w1
        self.params = _abi.make_channel_params(W, cols.get("bias", 0.0), cols.get("sigma", 0.0),
                                               cols.get("resolution", 0.0), delay, seed, row_offset, DT, tau_diff)
        self.state = {"counter": a.DeviceArray((B,), np.int32).zero_()}
        if delay:
            self.state["ring"] = _nan_filled((delay + 1, B, W), dtype)
        if difference:
            self.state["prev"], self.state["d_f"] = _nan_filled((B, W), dtype), _nan_filled((B, W), dtype)
        self.in0, self.in1 = a.DeviceArray((B, w0), dtype), (a.DeviceArray((B, w1), dtype) if w1 else None)

    def tick(self, x):
        x = np.asarray(x, dtype=self.dtype)
        self.in0.copy_from_numpy(x[:, :self.w0])
        if self.w1:
            self.in1.copy_from_numpy(x[:, self.w0:])
        ret = sensing.channel_step(self.params, self.in0, self.state, in1=self.in1, dy=self.difference,
                                   dtype=self.dtype)
        ret = [r.numpy() for r in (ret if isinstance(ret, tuple) else (ret,))]
        dy = ret.pop() if self.difference else None
        return np.concatenate(ret, axis=1), dy


def _reference(kind, B, W, dtype, delay, difference):
    """-> (outs [K,B,W], dys, largest |g|, v / resolution of every tick)"""
    ref = channel_ref.ChannelRef(W, B, delay=delay, difference=difference, tau_diff=TAU, dt=DT, seed=SEED, dtype=dtype,
                                 **_columns(kind, W))
    outs, dys, gmax = [], [], 0.0
    for t in range(K):
        o, d = ref.tick(_inputs()[t, :B, :W], n=_normals(SEED)[:B, t, :W])
        outs.append(o), dys.append(d)
        if difference:
            gmax = max(gmax, float(np.abs(ref.g).max()))
    return np.array(outs), dys, gmax, np.array(ref.v_hist)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("difference", [False, True])
@pytest.mark.parametrize("delay", [0, 1, 3])
@pytest.mark.parametrize("split", SPLITS)
def test_a_eight_ticks_match_the_reference(split, delay, difference, dtype):
    w0, w1 = split
    W = w0 + w1
    f32 = np.dtype(dtype) == np.float32
    worst = {}
    for B in BATCHES:
        for kind in ("mixed", "encoder"):
            cols = _columns(kind, W)
            outs, dys, gmax, scaled = _reference(kind, B, W, dtype, delay, difference)
            if kind == "encoder":  # no rounding decision of the reference is near a tie
                frac = np.abs(scaled - np.floor(scaled) - 0.5)
                assert frac.min() >= 1e-9, (B, frac.min())
            g = GpuChannel(w0, w1, B, dtype, delay, difference, TAU, SEED, **cols)
            for t in range(K):
                got, dy = g.tick(_inputs()[t, :B, :W])
                noisy = (cols["sigma"] > 0) & (cols["resolution"] == 0)
                assert np.array_equal(got[:, ~noisy], outs[t][:, ~noisy]), (kind, B, t)
                if noisy.any():
                    bound = 256 * EPS64 * cols["sigma"][noisy] + (EPS32 * np.abs(outs[t][:, noisy]) if f32 else 0.0)
                    err = np.abs(got[:, noisy].astype(np.float64) - outs[t][:, noisy])
                    worst["noise / bound"] = max(worst.get("noise / bound", 0.0), float((err / bound).max()))
                    assert (err <= bound).all(), (kind, B, t, float((err / bound).max()))
                if difference:
                    err = float(np.abs(dy.astype(np.float64) - dys[t]).max())
                    worst["dy / |g|max"] = max(worst.get("dy / |g|max", 0.0), err / gmax)
                    if t == 0:
                        assert not dy.any()
            if difference:
                assert gmax > 0 and worst["dy / |g|max"] <= (1e-5 if f32 else 1e-12), (kind, B, worst)
            assert g.state["counter"].numpy().tolist() == [K] * B
    print(split, delay, difference, np.dtype(dtype).name, worst)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_b_transparent_is_the_identity_and_without_noise_the_seed_changes_nothing(dtype):
    B, (w0, w1) = 65, (9, 7)
    x = (np.random.RandomState(8).standard_normal((B, 16)) * 10.0 ** np.arange(-8, 8)).astype(dtype)
    g = GpuChannel(w0, w1, B, dtype, seed=99)
    for _ in range(2):
        got, _ = g.tick(x)
        assert got.tobytes() == x.tobytes()
    cols = dict(bias=0.01, resolution=np.where(np.arange(16) % 2, 1e-3, 0.0))
    runs = []
    for seed in (1, 2 ** 63 + 5):
        g = GpuChannel(w0, w1, B, dtype, delay=1, difference=True, seed=seed, **cols)
        runs.append([g.tick(x * (t + 1)) for t in range(3)])
    for (o1, d1), (o2, d2) in zip(*runs):
        assert o1.tobytes() == o2.tobytes() and d1.tobytes() == d2.tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_c_a_rows_bits_do_not_depend_on_the_batch_and_views_may_be_unaligned(dtype):
    w0, w1, lo, hi = 7, 3, 300, 364
    W = w0 + w1
    cols = dict(sigma=0.3, resolution=np.where(np.arange(W) % 2, ENCODER, 0.0))
    whole = GpuChannel(w0, w1, BMAX, dtype, delay=3, difference=True, tau_diff=TAU, seed=SEED, **cols)
    part = GpuChannel(w0, w1, hi - lo, dtype, delay=3, difference=True, tau_diff=TAU, seed=SEED, row_offset=lo, **cols)
    # the part's arrays are row views one row into larger buffers: 7 and 3 elements past an aligned address
    bufs = {"in0": a.DeviceArray((hi - lo + 1, w0), dtype), "in1": a.DeviceArray((hi - lo + 1, w1), dtype)}
    part.in0, part.in1 = bufs["in0"].rows(1, hi - lo + 1), bufs["in1"].rows(1, hi - lo + 1)
    for name in ("prev", "d_f"):
        bufs[name] = _nan_filled((hi - lo + 1, W), dtype)
        part.state[name] = bufs[name].rows(1, hi - lo + 1)
    for t in range(5):
        x = _inputs()[t, :, :W]
        (o1, d1), (o2, d2) = whole.tick(x), part.tick(x[lo:hi])
        assert np.abs(o1 - x).max() > 0
        assert o1[lo:hi].tobytes() == o2.tobytes() and d1[lo:hi].tobytes() == d2.tobytes(), t
    # and the numbering is the reference's: the part's first output is the reference's rows 300..363
    ref = channel_ref.ChannelRef(W, hi - lo, seed=SEED, row_offset=lo, dtype=dtype, sigma=0.3, resolution=0.0)
    g = GpuChannel(w0, w1, hi - lo, dtype, seed=SEED, row_offset=lo, sigma=0.3)
    x = _inputs()[0, lo:hi, :W]
    err = np.abs(g.tick(x)[0].astype(np.float64) - ref.tick(x)[0])
    assert (err <= 256 * EPS64 * 0.3 + (EPS32 * 4.0 if np.dtype(dtype) == np.float32 else 0.0)).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_d_graph_replay_equals_single_launches(dtype):
    B, W = 130, 12
    stream = a.Stream(0)
    x = a.DeviceArray.from_numpy(_inputs()[0, :B, :6].astype(dtype))
    x1 = a.DeviceArray.from_numpy(_inputs()[1, :B, :6].astype(dtype))
    kw = dict(noise_std=0.05, resolution=ENCODER, bias=1e-3, delay=3, difference=True, tau_diff=TAU, seed=5, dtype=dtype,
              stream=stream)
    one, many = a.SignalChannel(W, B, **kw), a.SignalChannel(W, B, **kw)
    for _ in range(K):
        r1 = one.apply(x, x1)
    with engine.Plan(device=0, stream=stream) as plan:
        r2 = many.apply(x, x1)
    plan.launch_graph(K)
    assert len(r1) == len(r2) == 3
    for u, v in zip(r1, r2):
        hu = u.numpy(stream)
        assert np.isfinite(hu).all() and hu.tobytes() == v.numpy(stream).tobytes()
    assert r1[2].numpy(stream).any()
    s1, s2 = one.device_state(), many.device_state()
    assert sorted(s1) == ["counter", "d_f", "prev", "ring"]
    for k in s1:
        assert s1[k].numpy(stream).tobytes() == s2[k].numpy(stream).tobytes(), k
    assert one.ticks().tolist() == [K] * B
    # reset(rows): those rows start again, the others go on
    many.reset((10, 20))
    plan.launch_graph(K)
    assert many.ticks().tolist() == [2 * K] * 10 + [K] * 10 + [2 * K] * (B - 20)
    with pytest.raises(ValueError):
        many.apply(x)  # six columns for a channel of twelve
    plan.close()


def test_e_statistics_of_the_devices_normals():
    from tests.test_channel_hostsim import STAT_COLS, STAT_ROWS, STAT_SEED, STAT_TICKS

    ch = a.SignalChannel(STAT_COLS, STAT_ROWS, noise_std=1.0, seed=STAT_SEED)
    zero = a.DeviceArray((STAT_ROWS, STAT_COLS)).zero_()
    got = np.stack([ch.apply(zero).numpy() for _ in range(STAT_TICKS)], axis=1)
    assert got.size == 393216
    z = channel_ref.statistics(got)
    print({k: round(float(v), 2) for k, v in z.items()})
    assert all(abs(v) <= 4 for v in z.values()), z
    n = channel_ref.normal_block(STAT_SEED, np.arange(STAT_ROWS), np.arange(STAT_TICKS), np.arange(STAT_COLS))
    assert np.abs(got - n).max() <= 256 * EPS64


def test_f_closed_loop_with_transparent_and_delayed_sensing():
    from abr_control_amd.arms import ur5

    B, T = 64, 50
    rc = ur5.Config()
    n = rc.N_JOINTS
    rng = np.random.RandomState(9)
    q0 = rng.uniform(-1.0, 1.0, (B, n))
    target = np.zeros((B, 6))
    target[:, :3] = rc.Tx("EE", q0 + 0.1)
    law = _abi.make_osc_params(n, kp=200, use_C=True, use_g=True)
    plant = _abi.make_plant_params(DT, substeps=2)
    stream = a.Stream(0)

    def loop(sensor_kw, actuator):
        """-> (recorded q at the start of every tick, recorded q_meas or None, recorded q after every tick)"""
        q, dq, tgt = (a.DeviceArray.from_numpy(x) for x in (q0, np.zeros((B, n)), target))
        u = a.DeviceArray((B, n)).zero_(stream)
        rec = lambda: a.LoopRecorder(rc, B, capacity=T, columns=("q",), stats=False, stream=stream)
        before, meas, after = rec(), rec(), rec()
        sensor = None if sensor_kw is None else a.JointSensor(rc, B, dt=DT, stream=stream, **sensor_kw)
        act = a.SignalChannel(n, B, dt=DT, stream=stream) if actuator else None
        with engine.Plan(device=0, stream=stream) as tick:
            before.record(q, None, None, None)
            qm, dqm = (q, dq) if sensor is None else sensor.measure(q, dq)
            if sensor is not None:
                meas.record(qm, None, None, None)
            engine.osc_generate(rc.arm_id, n, law, qm, dqm, tgt, u=u, stream=stream)
            engine.plant_step(rc.arm_id, n, plant, q, dq, u if act is None else act.apply(u), stream=stream)
            after.record(q, None, None, None)
        tick.launch_graph(T)
        out = (before.history()["q"], meas.history()["q"] if sensor is not None else None, after.history()["q"])
        tick.close()
        return out

    _, _, plain = loop(None, False)
    assert plain.shape == (T, B, n) and np.isfinite(plain).all() and np.abs(plain[-1] - q0).max() > 1e-3
    _, qm, with_channels = loop({}, True)
    assert with_channels.tobytes() == plain.tobytes()
    before, qm, delayed = loop(dict(delay=2), False)
    assert np.isfinite(delayed).all() and delayed.tobytes() != plain.tobytes()
    for t in range(T):
        assert qm[t].tobytes() == before[max(t - 2, 0)].tobytes(), t
