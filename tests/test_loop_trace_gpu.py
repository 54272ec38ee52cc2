"""The loop recorder on the GPU (abrk_loop_trace_batch, engine.loop_trace, LoopRecorder): the host-build cases of
tests/trace_cases.py through the device for compile-time, runtime-table and plugin kernels, batch edges either side of a
wavefront, rows restarted inside a wavefront (where the cooperative history store must fall back), capacity and
decimation, and the recorded closed loop { path_next; OSC; plant_step; record } against the same ticks issued by the
host."""
import importlib.util
import os

import numpy as np
import pytest

from abr_control_amd import _abi
from tests import trace_cases as tc
from tests.conftest import REPO

pytestmark = pytest.mark.gpu
BATCHES = (1, 63, 64, 65, 130)
_cache = {}


def cfg(name):
    """-> (robot_config, table, arm key of trace_cases.LINK_FRAME)"""
    if name not in _cache:
        from abr_control_amd import arms
        from tests import compiled_arms

        if name in _abi.BUILTIN_ARMS:
            _cache[name] = (getattr(arms, name).Config(), _abi.load_table(name), name)
        elif name == "ur5_rt":
            tab = _abi.load_table("ur5")
            _cache[name] = (arms.from_table(tab, compiled=False), tab, "ur5")
        else:
            assert name == "synthetic4_compiled"
            tab = compiled_arms.test_arms()["synthetic4"]
            rc = arms.from_table(tab)
            assert rc.plugin_path, "no synthetic4 plugin for the current headers - run build()"
            _cache[name] = (rc, tab, "synthetic4")
    return _cache[name]


def host_tick(rc):
    """one tick on NumPy arrays through the library's staging"""
    from abr_control_amd import engine

    def tick(p, q, dq, u, tg, counter, hist, st, se, dtype):
        engine.loop_trace(rc.arm_id, rc.N_JOINTS, p, q, dq, u, tg, counter, hist, st, se, dtype=dtype)

    return tick


def device_run(rc, dtype, src, mask, every, capacity, tol, frame_id, x_off, ticks=None):
    """tc.run with every array resident on the device and the ticks enqueued back to back on one stream"""
    import abr_control_amd as a
    from abr_control_amd import engine

    dt = np.dtype(dtype)
    n = rc.N_JOINTS
    T, B = src[0].shape[:2]
    ticks = T if ticks is None else ticks
    s = a.Stream(0)
    W = _abi.trace_layout(mask, n)[1]
    p = _abi.make_trace_params(frame_id, x_off, every, capacity, mask, tol)
    dev = [[a.DeviceArray.from_numpy(np.ascontiguousarray(x[t], dtype=dt)) for x in src] for t in range(ticks)]
    hist = a.DeviceArray.from_numpy(np.full((capacity, B, W), tc.SENTINEL, dt))
    # (zero fills on the stream that consumes them)
    st, se = a.DeviceArray((B, 4)).zero_(s), a.DeviceArray((B,), np.int32).zero_(s)
    counter = a.DeviceArray((B,), np.int32).zero_(s)
    for t in range(ticks):
        engine.loop_trace(rc.arm_id, n, p, *dev[t], counter, hist, st, se, dtype=dt, stream=s)
    return hist.numpy(s), st.numpy(s), se.numpy(s), counter.numpy(s)


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("which", tc.FRAMES)
@pytest.mark.parametrize("name", ("ur5", "jaco2", "twojoint", "ur5_rt", "synthetic4_compiled"))
def test_gpu_loop_trace_parity(name, which, dtype):
    """the host-build cases on the device (fp32: the history is float32, the statistics float64)"""
    rc, table, arm = cfg(name)
    tc.check_case(host_tick(rc), table, arm, which, dtype)


_alone = {}


def rows_alone(cols, every, capacity, T, resets_of=lambda b: ()):
    """UR5 fp64: every row of the 130-row inputs run ALONE (B = 1), once per configuration -> per-row
    (history [capacity, W], stats [4], settle, counter)"""
    key = (cols, every, capacity, T, tuple(resets_of(b) for b in range(BATCHES[-1])))
    if key not in _alone:
        rc = cfg("ur5")[0]
        tick = host_tick(rc)
        src = tc.inputs(6, BATCHES[-1], T=T)
        mask = _abi.trace_columns_mask(cols)
        out = []
        for b in range(BATCHES[-1]):
            h, st, se, c = tc.run(tick, 6, np.float64, tuple(x[:, b:b + 1] for x in src), mask, every, capacity, 0.6,
                                  _abi.frame_id("EE", 6), None, resets=resets_of(b))
            out.append((h[:, 0], st[0], se[0], c[0]))
        _alone[key] = out
    return _alone[key]


@pytest.mark.parametrize("cols", (tc.ALL, ("q", "xyz")), ids=("W28", "W9"))
@pytest.mark.parametrize("B", BATCHES)
def test_gpu_loop_trace_batch_edges_and_bit_independence(B, cols):
    """every row of a batch equals the same row run alone, bit for bit, and nothing is written out of place: the slots
    past the last tick keep their fill.  (W = 9 with an odd batch: every other slot starts off a 16-byte boundary.)"""
    rc = cfg("ur5")[0]
    T, cap = 5, 7
    src = tuple(x[:, :B] for x in tc.inputs(6, BATCHES[-1], T=T))
    mask = _abi.trace_columns_mask(cols)
    h, st, se, c = device_run(rc, np.float64, src, mask, 1, cap, 0.6, _abi.frame_id("EE", 6), None)
    alone = rows_alone(cols, 1, cap, T)
    for b in range(B):
        ha, sta, sea, ca = alone[b]
        assert np.array_equal(h[:, b], ha) and np.array_equal(st[b], sta) and se[b] == sea and c[b] == ca == T, b
    assert (h[T:] == tc.SENTINEL).all() and not (h[:T] == tc.SENTINEL).any()


def test_gpu_loop_trace_restarted_rows_inside_a_wavefront():
    """B = 70; rows 10..39 restarted after 4 ticks, every = 2: they write slots 0, 1 again while their neighbours write
    slots 2, 3 - one wavefront, two slots.  Every row equals its own single-row run with the same schedule."""
    import abr_control_amd as a
    from abr_control_amd import LoopRecorder

    rc = cfg("ur5")[0]
    B, T = 70, 8
    src = tuple(x[:, :B] for x in tc.inputs(6, BATCHES[-1], T=T))
    s = a.Stream(0)
    rec = LoopRecorder(rc, B, capacity=4, every=2, columns=tc.ALL, tol=0.6, stream=s)
    dev = [[a.DeviceArray.from_numpy(np.ascontiguousarray(x[t]), stream=s.ptr) for x in src] for t in range(T)]
    for t in range(T):
        if t == 4:
            rec.reset(rows=(10, 40))
        rec.record(*dev[t])
    h = rec.device_history().numpy(s)
    ds = rec.device_stats()
    st, se, c = ds["stats"].numpy(s), ds["settle"].numpy(s), ds["counter"].numpy(s)
    alone = rows_alone(tc.ALL, 2, 4, T, resets_of=lambda b: ((4, 0, 1),) if 10 <= b < 40 else ())
    for b in range(B):
        ha, sta, sea, ca = alone[b]
        written = ha != tc.SENTINEL
        assert written.all(axis=1).sum() == (2 if 10 <= b < 40 else 4)
        assert np.array_equal(h[:, b][written], ha[written]) and np.isnan(h[:, b][~written]).all(), b
        assert np.array_equal(st[b], sta) and se[b] == sea and c[b] == ca == (4 if 10 <= b < 40 else 8), b
    # the host views: NaN where a row has not written since its reset
    hist = rec.history()
    assert hist["q"].shape == (4, B, 6) and hist["err"].shape == (4, B, 1)
    assert np.isnan(hist["xyz"][2:, 10:40]).all() and not np.isnan(hist["xyz"][:, :10]).any()
    assert np.array_equal(rec.stats()["ticks"], c)


def test_gpu_loop_trace_capacity_and_decimation():
    """every = 3, capacity = 4, 14 ticks: slots at ticks 0, 3, 6, 9, tick 12 dropped; the statistics cover all 14 ticks;
    the history-only and the statistics-only forms compute the same and leave the other's buffers alone"""
    rc = cfg("ur5")[0]
    B, T = 70, 14
    src = tuple(x[:, :B] for x in tc.inputs(6, BATCHES[-1], T=T))
    mask = _abi.trace_columns_mask(tc.ALL)
    fid = _abi.frame_id("EE", 6)
    full = device_run(rc, np.float64, src, mask, 1, T, 0.6, fid, None)
    h, st, se, c = device_run(rc, np.float64, src, mask, 3, 4, 0.6, fid, None)
    assert np.array_equal(h, full[0][[0, 3, 6, 9]])
    err = tc.columns(full[0], mask, 6)["err"][..., 0]
    tc.check_stats(st, se, c, err, 0.6)
    tick = host_tick(rc)
    ho = tc.run(tick, 6, np.float64, src, mask, 3, 4, 0.6, fid, None, stats=False)
    assert ho[1] is None and ho[2] is None and np.array_equal(ho[0], h) and np.array_equal(ho[3], c)
    so = tc.run(tick, 6, np.float64, src, mask, 3, 4, 0.6, fid, None, history=False)
    assert so[0] is None and np.array_equal(so[1], st) and np.array_equal(so[2], se)


def test_gpu_recorded_closed_loop_history_equals_host_ticks():
    """{ path_next; OSC(use_C, target_velocity); plant_step; record } recorded once and replayed with launch_graph(40)
    against the same three calls issued tick by tick from the host with q, dq, u, target copied back after each"""
    import abr_control_amd as a
    from abr_control_amd import LoopRecorder, engine
    from abr_control_amd.controllers.path_planners import PathPlanner, position_profiles, velocity_profiles

    rc = cfg("ur5")[0]
    n, B, K, dt = 6, 70, 40, 0.001
    q0 = np.random.RandomState(3).uniform(-1.0, 1.0, (B, n))
    stream = a.Stream(0)
    planner = PathPlanner(position_profiles.Linear(), velocity_profiles.Gaussian(dt=dt, acceleration=2), stream=stream)
    planner.generate_path(rc.Tx("EE", q0), rc.Tx("EE", q0 + 0.2), max_velocity=1.0,
                          start_orientation=np.zeros((B, 3)), target_orientation=np.zeros((B, 3)), to_host=False)
    path, n_timesteps = planner.device_path()
    law = _abi.make_osc_params(n, kp=200, use_C=True, use_g=True)
    plant = _abi.make_plant_params(dt, substeps=1, gravity=True)
    q, dq, u, tgt, tgt_v = (a.DeviceArray((B, w)) for w in (n, n, n, 6, 6))
    counter = a.DeviceArray((B,), np.int32)
    tol = 0.01
    rec = LoopRecorder(rc, B, capacity=K, columns=tc.ALL, tol=tol, stream=stream)

    def restart():
        q.copy_from_numpy(q0, stream)
        for arr in (dq, u, tgt, tgt_v, counter):
            arr.zero_(stream)
        rec.reset()

    def three_calls():
        engine.path_next(path, n_timesteps, counter, tgt, tgt_v, stream=stream)
        engine.osc_generate(rc.arm_id, n, law, q, dq, tgt, target_velocity=tgt_v, u=u, stream=stream)
        engine.plant_step(rc.arm_id, n, plant, q, dq, u, stream=stream)

    restart()
    host = {k: [] for k in ("q", "dq", "u", "target")}
    for _ in range(K):
        three_calls()
        for k, arr in zip(("q", "dq", "u", "target"), (q, dq, u, tgt)):
            host[k].append(arr.numpy(stream))
    with engine.Plan(device=0, stream=stream) as tick:
        three_calls()
        rec.record(q, dq, u, tgt)
    restart()
    tick.launch_graph(K)
    hist = rec.history()
    raw = rec.device_history().numpy(stream)
    for k in host:
        assert np.array_equal(hist[k], np.array(host[k])), k
    st = rec.stats()
    ds = rec.device_stats()
    tc.check_stats(ds["stats"].numpy(stream), ds["settle"].numpy(stream), ds["counter"].numpy(stream),
                   hist["err"][..., 0], tol)
    e = hist["err"][..., 0]
    assert np.array_equal(st["err_last"], e[-1]) and np.array_equal(st["ticks"], np.full(B, K))
    assert np.allclose(st["err_rms"], np.sqrt((e * e).mean(axis=0)), rtol=1e-12, atol=0)
    assert np.array_equal(st["settle_tick"], tc.settle_ref(e, tol) - 1)
    d = hist["target"][..., :3] - hist["xyz"]
    assert (np.abs(e - np.linalg.norm(d, axis=-1)) <= 8 * np.finfo(float).eps * e).all()
    restart()
    for _ in range(K):
        tick.launch()
    assert np.array_equal(rec.device_history().numpy(stream), raw), "launch() x K and launch_graph(K) differ"


def test_gpu_path_following_example_reports_from_one_replay():
    spec = importlib.util.spec_from_file_location(
        "path_following_ur5_headless", os.path.join(REPO, "examples", "path_following_ur5_headless.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(256)
