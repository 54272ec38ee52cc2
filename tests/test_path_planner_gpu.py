"""The batched path planner on the GPU: every fixture case against the reference's own PathPlanner (step counts exact,
all columns within tests/path_cases.BOUND, padding equal to the last point), the edge group of all 24 Euler sequences,
SLERP branches and special directions included; the orientation columns of every sequence against rotations composed in
NumPy; rows independent of their batch bit for bit at 63 / 64 / 65 / 70 rows, also where one batch mixes rows of one,
two and three workgroup strides; the LDS and the global-scratch forms of the fill pass, the path feed recorded into a
Plan, a closed loop { path_next; OSC; plant_step } replayed as a graph against the same calls fed from the host, the
error path of a row without a path (start == target, a movement exactly towards -(1,1,1)/sqrt(3)) and a t_max below a
row's step count.  Maxima observed on an MI355X: DESIGN.md "Path planner"."""
import functools

import numpy as np
import pytest

from abr_control_amd import _abi
from abr_control_amd.controllers.path_planners import PathPlanner, position_profiles, velocity_profiles
from tests import path_cases

pytestmark = pytest.mark.gpu


def _planner(name, **kw):
    pos, vel = path_cases.profiles(name, **kw)
    return PathPlanner(pos, vel, axes=path_cases.rows(name)["axes"])


def _draw(name, B, seed):
    """B rows with the settings of a fixture case: start in +-0.4, direction uniform on the sphere, the case's lengths.
    'ragged' (dt = 0.001): the three fixture rows - under 64, 257-511 and over 512 steps - then B - 3 rows of 0.0025-0.25 m"""
    meta, _ = path_cases.golden(name)
    fixed = path_cases.rows(name) if name == "ragged" else None
    lo, hi = (0.0025, 0.25) if fixed else meta["cases"][name]["length"]
    r = np.random.RandomState(seed)
    n = B - 3 if fixed else B
    start = r.uniform(-0.4, 0.4, (n, 3))
    d = r.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = start, start + d * r.uniform(lo, hi, (n, 1)), r.uniform(-1, 1, (n, 3)), r.uniform(-1, 1, (n, 3))
    if fixed:
        out = tuple(np.concatenate([f, o]) for f, o in zip((fixed["start"], fixed["target"], fixed["so"], fixed["to"]), out))
    return out


@pytest.mark.parametrize("name", path_cases.names())
def test_gpu_fixture_cases(name):
    """(a) the batch of a case's rows, and its first row as one movement"""
    r = path_cases.rows(name)
    planner = _planner(name)
    path = planner.generate_path(r["start"], r["target"], start_orientation=r["so"], target_orientation=r["to"],
                                 **r["kwargs"])
    W = 6 if r["so"] is None else 12
    assert path.shape == (len(r["nt"]), r["nt"].max(), W) and planner.n_timesteps.shape == (len(r["nt"]),)
    path_cases.check_against_reference(name, path, planner.n_timesteps, lambda what, v: print(f"gpu {what}: {v:.3e}"))
    assert np.array_equal(planner.time_to_converge, r["nt"] * planner.dt)
    assert np.array_equal(planner.position_path, path[..., :3]) and np.array_equal(planner.velocity_path, path[..., 3:6])
    # next() / next_at_n(): every row clamps at its own last point
    last = path[np.arange(len(path)), r["nt"] - 1]
    assert np.array_equal(planner.next(), path[:, 0]) and np.array_equal(planner.next(), path[:, 1])
    assert np.array_equal(planner.next_at_n(10 ** 6), last) and np.array_equal(planner.next_at_n(3), path[:, 3])
    for _ in range(int(r["nt"].max())):
        planner.next()
    assert np.array_equal(planner.next(), last) and np.array_equal(planner.n, r["nt"] - 1)
    # one movement: the reference's shapes
    one = planner.generate_path(r["start"][0], r["target"][0], start_orientation=None if r["so"] is None else r["so"][0],
                                target_orientation=None if r["to"] is None else r["to"][0], **r["kwargs"])
    assert one.shape == (r["nt"][0], W) and planner.n_timesteps == r["nt"][0] and planner.n == 0
    assert np.array_equal(one, path[0, :r["nt"][0]])
    assert np.array_equal(planner.next(), one[0]) and np.array_equal(planner.next_at_n(10 ** 6), one[-1])
    if W == 12:
        assert np.array_equal(planner.orientation_path, one[:, 6:9]) and planner.ang_velocity_path.shape == (len(one), 3)


@pytest.mark.parametrize("name", path_cases.MAIN + ("ragged",))
def test_gpu_rows_do_not_depend_on_their_batch_bitwise(name):
    """(b) 70 ragged rows with a case's settings: every row equals its own single-row run bit for bit, and so do the
    rows of the 63-, 64- and 65-row batches (either side of a wavefront of the plan pass).  'ragged': rows shorter than
    a wavefront beside rows of two and of three workgroup strides, so the padding is wider than a stride"""
    start, target, so, to = _draw(name, 70, 70)
    kw = path_cases.rows(name)["kwargs"]
    planner = _planner(name)
    full = planner.generate_path(start, target, start_orientation=so, target_orientation=to, **kw).copy()
    nt = planner.n_timesteps.copy()
    assert nt.min() >= 2 and len(set(nt.tolist())) > 20  # ragged
    if name == "ragged":
        assert np.array_equal(nt[:3], path_cases.rows(name)["nt"]) and nt[0] < 64 and 256 < nt[1] < 512 < nt[2]
        assert nt.max() - nt.min() > 256
    for b in range(70):
        one = planner.generate_path(start[b], target[b], start_orientation=so[b], target_orientation=to[b], **kw)
        assert planner.n_timesteps == nt[b] and np.array_equal(one, full[b, :nt[b]]), b
        assert np.array_equal(full[b, nt[b]:], np.broadcast_to(full[b, nt[b] - 1], full[b, nt[b]:].shape)), b
    for B in (63, 64, 65):
        part = planner.generate_path(start[:B], target[:B], start_orientation=so[:B], target_orientation=to[:B], **kw)
        assert np.array_equal(planner.n_timesteps, nt[:B])
        t = part.shape[1]
        assert t == nt[:B].max() and np.array_equal(part, full[:B, :t])


@functools.lru_cache(maxsize=None)
def _hostsim_line(S):
    from tests import hostsim_path

    start, target, so, to = _draw("case1", 5, 11)
    vel = velocity_profiles.Gaussian(dt=0.004, acceleration=4)
    return (start, target, so, to) + hostsim_path.generate_path(position_profiles.Linear(n_sample_points=S), vel, start,
                                                                target, 1.0, so, to)


@pytest.mark.parametrize("S", (2, 10, 200, 1000, 8200))
def test_gpu_sample_counts_lds_and_global_scratch(S):
    """(c) Linear(n_sample_points=S): dist_steps in LDS up to 8192 samples, searched in global memory beyond, against
    the same row program on the host (itself held to the reference by tests/test_path_planner_hostsim.py)"""
    start, target, so, to, ref, ref_nt = _hostsim_line(S)
    planner = PathPlanner(position_profiles.Linear(n_sample_points=S), velocity_profiles.Gaussian(dt=0.004, acceleration=4))
    path = planner.generate_path(start, target, 1.0, start_orientation=so, target_orientation=to)
    assert np.array_equal(planner.n_timesteps, ref_nt) and path.shape == ref.shape
    d = np.abs(path - ref).max(axis=(0, 1))
    print(f"gpu vs hostsim S={S}: position {d[:3].max():.3e} velocity {d[3:6].max():.3e} euler {d[6:9].max():.3e} "
          f"angular velocity {d[9:].max():.3e}")
    assert d.max() < path_cases.BOUND
    # a straight line is the same line whatever its sampling
    assert np.abs(path - _hostsim_line(10)[4]).max() < path_cases.BOUND


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("name", ("case4", "wide6"))
def test_gpu_path_next_recorded_in_a_plan(name, dtype):
    """(d) K launches of { path_next } as one graph, K beyond the shortest row's path: counters clamp per row, the target
    buffers hold path[b, min(K - 1, T - 1)] - cast to the loop's type, nothing else; a 6-wide path leaves the
    orientation columns alone"""
    import abr_control_amd as a
    from abr_control_amd import engine

    r = path_cases.rows(name)
    planner = _planner(name)
    path = planner.generate_path(r["start"], r["target"], start_orientation=r["so"], target_orientation=r["to"],
                                 **r["kwargs"])
    nt = r["nt"]
    K = int(nt.min()) + 9
    assert nt.min() < K < nt.max() + 9
    B, W = path.shape[0], path.shape[2]
    path_d, nt_d = planner.device_path()
    s = a.Stream(0)
    counter = a.DeviceArray((B,), np.int32).zero_(s)
    mark = np.full((B, 6), -7.0, dtype)
    tgt, tv = a.DeviceArray.from_numpy(mark), a.DeviceArray.from_numpy(mark)
    with engine.Plan(device=0, stream=s) as plan:
        engine.path_next(path_d, nt_d, counter, tgt, tv, dtype=dtype, stream=s)
    plan.launch_graph(K)
    s.sync()
    assert np.array_equal(counter.numpy(s), np.minimum(K, nt - 1))
    point = path[np.arange(B), np.minimum(K - 1, nt - 1)]
    want_t, want_v = mark.copy(), mark.copy()
    want_t[:, :3], want_v[:, :3] = point[:, 0:3], point[:, 3:6]
    if W == 12:
        want_t[:, 3:], want_v[:, 3:] = point[:, 6:9], point[:, 9:12]
    assert np.array_equal(tgt.numpy(s), want_t) and np.array_equal(tv.numpy(s), want_v)
    # host arrays, without target_velocity: one step per call
    c, t = np.zeros(B, np.int32), mark.copy()
    engine.path_next(path, planner.n_timesteps.astype(np.int32), c, t, dtype=dtype)
    assert np.array_equal(c, np.ones(B)) and np.array_equal(t[:, :3], path[:, 0, :3].astype(dtype))


def test_gpu_closed_loop_follows_the_path_as_a_graph():
    """(e) UR5, 130 arms, 40 ticks of { path_next; OSC with target_velocity; plant_step } recorded once and replayed as
    one graph, against the same three engine calls issued tick by tick with PathPlanner.next() feeding the targets from
    the host: bit for bit"""
    import abr_control_amd as a
    from abr_control_amd import engine
    from abr_control_amd.arms import ur5

    rc = ur5.Config()
    B, K = 130, 40
    r = np.random.RandomState(5)
    q0 = r.uniform(-1.0, 1.0, (B, 6))
    ee = engine.dynamics(rc.arm_id, 6, q0, want=("Tx",))["Tx"]
    d = r.normal(size=(B, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    target = ee + d * r.uniform(0.05, 0.15, (B, 1))
    planner = PathPlanner(position_profiles.Linear(), velocity_profiles.Gaussian(dt=0.001, acceleration=4))
    planner.generate_path(ee, target, 1.0, start_orientation=r.uniform(-1, 1, (B, 3)),
                          target_orientation=r.uniform(-1, 1, (B, 3)))
    assert planner.n_timesteps.min() > K
    p = _abi.make_osc_params(6, kp=200, use_C=True, use_g=True)
    pp = _abi.make_plant_params(1e-3)
    s = a.Stream(0)
    mk = lambda x: a.DeviceArray.from_numpy(np.ascontiguousarray(x))
    z = np.zeros((B, 6))
    # tick by tick, fed from the host
    q_e, dq_e, u_e, t_e, v_e = mk(q0), mk(z), mk(z), mk(z), mk(z)
    for _ in range(K):
        point = planner.next()
        t_e.copy_from_numpy(point[:, [0, 1, 2, 6, 7, 8]], s)
        v_e.copy_from_numpy(point[:, [3, 4, 5, 9, 10, 11]], s)
        engine.osc_generate(rc.arm_id, 6, p, q_e, dq_e, t_e, target_velocity=v_e, u=u_e, stream=s)
        engine.plant_step(rc.arm_id, 6, pp, q_e, dq_e, u_e, stream=s)
    s.sync()
    # the recorded tick
    path_d, nt_d = planner.device_path()
    counter = a.DeviceArray((B,), np.int32).zero_(s)
    q_g, dq_g, u_g, t_g, v_g = mk(q0), mk(z), mk(z), mk(z), mk(z)
    with engine.Plan(device=0, stream=s) as plan:
        engine.path_next(path_d, nt_d, counter, t_g, v_g, stream=s)
        engine.osc_generate(rc.arm_id, 6, p, q_g, dq_g, t_g, target_velocity=v_g, u=u_g, stream=s)
        engine.plant_step(rc.arm_id, 6, pp, q_g, dq_g, u_g, stream=s)
    plan.launch_graph(K)
    s.sync()
    for x, y in ((q_e, q_g), (dq_e, dq_g), (u_e, u_g), (t_e, t_g), (v_e, v_g)):
        assert np.array_equal(x.numpy(s), y.numpy(s))
    assert np.array_equal(counter.numpy(s), np.full(B, K)) and np.isfinite(q_g.numpy(s)).all()
    assert np.abs(q_g.numpy(s) - q0).max() > 1e-4  # the arms moved


@pytest.mark.parametrize("axes", sorted(_abi.EULER_AXES))
def test_gpu_orientation_columns_lie_on_the_geodesic(axes):
    """(g) no reference involved: the Euler columns of every sequence, turned into rotations by NumPy, start and end at
    the given orientations and walk the shorter geodesic between them at the fraction the position columns give"""
    start, target, so, to = path_cases.geodesic_rows(axes)
    planner = PathPlanner(position_profiles.Linear(), velocity_profiles.Gaussian(dt=path_cases.GEODESIC_DT, acceleration=4),
                          axes=axes)
    path = planner.generate_path(start, target, 1.0, start_orientation=so, target_orientation=to)
    path_cases.check_geodesic(axes, path, planner.n_timesteps, so, to, lambda line: print("gpu", line))


def test_gpu_no_path_exactly_towards_the_antidiagonal():
    """(h) a movement exactly towards -(1,1,1)/sqrt(3) (align_vectors divides by 1 + cs = 0; the reference raises) in a
    batch of four: ValueError, the same stream plans the next batch normally, and at the C ABI on host arrays
    n_timesteps marks that row alone"""
    import ctypes as C

    import abr_control_amd as a
    from abr_control_amd import engine
    from abr_control_amd._lib import PathError, lib
    from abr_control_amd.controllers.path_planners.path_planner import profile_tables

    start, target, so, to = path_cases.antidiagonal_batch()
    s = a.Stream(0)
    pos, vel = position_profiles.Linear(), velocity_profiles.Gaussian(dt=0.004, acceleration=4)
    planner = PathPlanner(pos, vel, stream=s)
    with pytest.raises(ValueError) as ei:
        planner.generate_path(start, target, 1.0, start_orientation=so, target_orientation=to)
    assert isinstance(ei.value, PathError) and ei.value.code == _abi.EPATH
    s.sync()  # reported once, by the call itself
    keep = [0, 1, 3]
    path = planner.generate_path(start[keep], target[keep], 1.0, start_orientation=so[keep], target_orientation=to[keep])
    nt = planner.n_timesteps.copy()
    assert nt.min() >= 2 and np.isfinite(path).all()
    assert np.abs(path[np.arange(3), nt - 1, :3] - target[keep]).max() < 0.01  # (the bound of the reference's own warning)
    table, off, cands = profile_tables(pos, vel, 1.0)
    P = _abi.PathParams(vel.dt, pos.n_sample_points, len(cands), 22, 12, table.size)
    with pytest.raises(PathError):
        engine.path_plan(P, table, off, start, target)
    nt4, rowplan, ds = np.full(4, -1, np.int32), np.zeros((4, 2), np.int32), np.zeros((4, pos.n_sample_points))
    rc = lib().abrk_path_plan_batch(C.byref(P), table.ctypes.data, off.ctypes.data, 4, start.ctypes.data,
                                    target.ctypes.data, nt4.ctypes.data, rowplan.ctypes.data, ds.ctypes.data, 0, None)
    assert rc == _abi.EPATH and nt4[2] == 0 and np.array_equal(nt4[keep], nt)
    # the fill passes leave that row alone and give the others what the batch of three got
    out = engine.path_fill(P, table, off, int(nt.max()), start, target, nt4, rowplan, ds, so, to)
    assert np.array_equal(out[keep], path)


def test_gpu_t_max_below_a_rows_step_count():
    """(i) engine.path_fill with t_max = max(n_timesteps) - 1 on the rows of case1, into a DeviceArray that holds a
    sentinel: a row that does not fit keeps the sentinel in every column (it used to get a truncated path without
    velocity columns), the others equal the normal call's rows cut at t_max bit for bit - and the host build of the row
    programs, which the device is to follow here, gives the same array"""
    import abr_control_amd as a
    from abr_control_amd import engine
    from abr_control_amd.controllers.path_planners.path_planner import profile_tables
    from tests import hostsim_path

    r = path_cases.rows("case1")
    pos, vel = path_cases.profiles("case1")
    table, off, cands = profile_tables(pos, vel, r["kwargs"]["max_velocity"])
    P = _abi.PathParams(vel.dt, pos.n_sample_points, len(cands), _abi.euler_axes_code(r["axes"]), 12, table.size)
    s = a.Stream(0)
    up = lambda h: a.DeviceArray.from_numpy(np.ascontiguousarray(h))
    d_table, d_start, d_target, d_so, d_to = up(table), up(r["start"]), up(r["target"]), up(r["so"]), up(r["to"])
    nt_d, rowplan_d, ds_d = engine.path_plan(P, d_table, off, d_start, d_target, stream=s)
    nt = nt_d.numpy(s)
    assert np.array_equal(nt, r["nt"])
    t_max = int(nt.max()) - 1
    B = len(nt)
    full = engine.path_fill(P, d_table, off, t_max + 1, d_start, d_target, nt_d, rowplan_d, ds_d, d_so, d_to, stream=s)
    cut = engine.path_fill(P, d_table, off, t_max, d_start, d_target, nt_d, rowplan_d, ds_d, d_so, d_to,
                           path=up(np.full((B, t_max, 12), -7.0)), stream=s)
    path_cases.check_truncated_fill(cut.numpy(s), full.numpy(s), nt, t_max, -7.0)
    model = hostsim_path.fill(pos, vel, r["start"], r["target"], r["so"], r["to"], t_max, sentinel=-7.0, **r["kwargs"])
    assert np.array_equal(model == -7.0, cut.numpy(s) == -7.0) and np.abs(model - cut.numpy(s)).max() < path_cases.BOUND


def test_gpu_row_without_a_path_raises_value_error():
    """(f) start == target in one row of a batch: ValueError (an error code - nothing faults), and the same stream plans
    the next batch as if nothing had happened; at the engine level n_timesteps marks the row"""
    import abr_control_amd as a
    from abr_control_amd import engine
    from abr_control_amd._lib import PathError
    from abr_control_amd.controllers.path_planners.path_planner import profile_tables

    r = path_cases.rows("case1")
    s = a.Stream(0)
    pos, vel = path_cases.profiles("case1")
    planner = PathPlanner(pos, vel, stream=s)
    target = r["target"].copy()
    target[2] = r["start"][2]
    with pytest.raises(ValueError) as ei:
        planner.generate_path(r["start"], target, start_orientation=r["so"], target_orientation=r["to"], **r["kwargs"])
    assert isinstance(ei.value, PathError) and ei.value.code == _abi.EPATH
    s.sync()  # reported once, by the call itself
    path = planner.generate_path(r["start"], r["target"], start_orientation=r["so"], target_orientation=r["to"],
                                 **r["kwargs"])
    path_cases.check_against_reference("case1", path, planner.n_timesteps, lambda *_: None)
    # a movement too short for every candidate is the reference's ValueError as well
    with pytest.raises(ValueError):
        planner.generate_path(r["start"][0], r["start"][0] + 1e-7, **r["kwargs"])
    # host arrays at the engine level: the call returns the code, n_timesteps is 0 for that row alone
    table, off, cands = profile_tables(pos, vel, 1.0)
    P = _abi.PathParams(vel.dt, pos.n_sample_points, len(cands), 22, 12, table.size)
    with pytest.raises(PathError):
        engine.path_plan(P, table, off, r["start"], target)
    nt, _, _ = engine.path_plan(P, table, off, r["start"], r["target"])
    assert np.array_equal(nt, r["nt"])
