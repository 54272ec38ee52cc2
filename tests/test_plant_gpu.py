"""The rigid-body plant on the GPU (abrk_forward_dynamics_batch, abrk_plant_step_batch, ArmSim) against the oracle
composed in NumPy (tests/plant_ref.py), plus the bitwise properties of the kernel and the closed loop as a recorded plan.
Batches: 1, 63, 64, 65 (either side of a wavefront) and 130 (a partial third wavefront)."""
import numpy as np
import pytest

from abr_control_amd import _abi
from tests.plant_ref import TOL_F32, TOL_F64, HostsimGiDyn, OracleDyn, Ref, draw, rel_err

pytestmark = pytest.mark.gpu
BATCHES = (1, 63, 64, 65, 130)
DTYPES = (np.float64, np.float32)


def _config(name):
    """-> (robot_config, reference)"""
    from abr_control_amd import arms
    from tests import compiled_arms, compiled_inertia_arms, compiled_plant_arms

    if name in _abi.BUILTIN_ARMS:
        tab = _abi.load_table(name)
        return getattr(arms, name).Config(), Ref(OracleDyn(tab))
    if name == "ur5_rt":
        tab = _abi.load_table("ur5")
        return arms.from_table(tab, compiled=False), Ref(OracleDyn(tab))
    if name == "ur5_compiled":
        tab = compiled_plant_arms.table()
        rc = arms.from_table(tab)
        assert rc.plugin_path, "no ur5_user plugin for the current headers - run build()"
        return rc, Ref(OracleDyn(tab))
    if name == "synthetic4_compiled":
        tab = compiled_arms.test_arms()["synthetic4"]
        rc = arms.from_table(tab)
        assert rc.plugin_path, "no synthetic4 plugin for the current headers - run build()"
        return rc, Ref(OracleDyn(tab))
    assert name.startswith("gi_")
    tab = compiled_inertia_arms.table(name[3:])
    return arms.from_table(tab), Ref(HostsimGiDyn(_abi.normalize_table(tab)))


_cache = {}


def cfg(name):
    if name not in _cache:
        _cache[name] = _config(name)
    return _cache[name]


def _fd(rc, q, dq, u, dtype, device_arrays=False):
    import abr_control_amd as a
    from abr_control_amd import engine

    n = rc.N_JOINTS
    if device_arrays:
        q, dq, u = (a.DeviceArray.from_numpy(np.ascontiguousarray(x, dtype=dtype)) for x in (q, dq, u))
        return engine.forward_dynamics(rc.arm_id, n, q, dq, u, dtype=dtype).numpy()
    return engine.forward_dynamics(rc.arm_id, n, q, dq, u, dtype=dtype)


def _step(rc, dt, sub, q, dq, u, dtype, device_arrays=False, calls=1, gravity=True):
    """`calls` plant steps -> (q, dq) as arrays of `dtype` (the inputs are left alone)"""
    import abr_control_amd as a
    from abr_control_amd import engine

    n = rc.N_JOINTS
    p = _abi.make_plant_params(dt, sub, gravity)
    q, dq, u = (np.array(x, dtype=dtype, order="C") for x in (q, dq, u))
    if device_arrays:
        qd, dqd, ud = (a.DeviceArray.from_numpy(x) for x in (q, dq, u))
        for _ in range(calls):
            engine.plant_step(rc.arm_id, n, p, qd, dqd, ud, dtype=dtype)
        return qd.numpy(), dqd.numpy()
    for _ in range(calls):
        engine.plant_step(rc.arm_id, n, p, q, dq, u, dtype=dtype)
    return q, dq


PARITY = ("twojoint", "threejoint", "ur5", "jaco2", "ur5_rt", "ur5_compiled", "synthetic4_compiled", "gi_synthetic4",
          "gi_ur5")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", PARITY)
def test_gpu_plant_parity(name, dtype):
    """ddq and one plant step (substeps 1 and 4), host arrays and DeviceArrays, every batch size.
    Worst measured over all cases: see profiles/plant_step.md."""
    rc, ref = cfg(name)
    n = rc.N_JOINTS
    tol = TOL_F64 if dtype == np.float64 else TOL_F32
    q, dq, u = draw(21, BATCHES[-1], n)
    ddq_ref = ref.ddq(q, dq, u)
    steps_ref = {sub: ref.steps(q, dq, u, 1e-3, sub) for sub in (1, 4)}
    worst = 0.0
    for B in BATCHES:
        for dev in (False, True):
            e = rel_err(_fd(rc, q[:B], dq[:B], u[:B], dtype, dev), ddq_ref[:B])
            worst = max(worst, e)
            assert e <= tol, (name, B, dev, e)
        for sub in (1, 4):
            qg, dqg = _step(rc, 1e-3, sub, q[:B], dq[:B], u[:B], dtype, device_arrays=B % 2 == 0)
            e = max(rel_err(qg, steps_ref[sub][0][:B]), rel_err(dqg, steps_ref[sub][1][:B]))
            worst = max(worst, e)
            assert e <= tol, (name, B, sub, e)
    print(f"plant parity {name} {np.dtype(dtype).name}: worst {worst:.2e}")


def test_gpu_plant_onejoint_is_singular():
    """the reference's one-joint arm has a massless link: M = [[0]], numpy's solve raises LinAlgError and so does the call"""
    rc, ref = cfg("onejoint")
    q, dq, u = draw(22, 65, 1)
    with pytest.raises(np.linalg.LinAlgError):
        ref.ddq(q, dq, u)
    for dtype in DTYPES:
        with pytest.raises(np.linalg.LinAlgError):
            _fd(rc, q, dq, u, dtype)
        with pytest.raises(np.linalg.LinAlgError):
            _step(rc, 1e-3, 1, q, dq, u, dtype)


@pytest.mark.parametrize("name", ("ur5", "jaco2"))
def test_gpu_plant_fifty_steps(name):
    """50 calls of 1 ms on DeviceArrays, B = 65, fp64, against the NumPy loop.  Worst measured: profiles/plant_step.md."""
    rc, ref = cfg(name)
    q, dq, u = draw(23, 65, rc.N_JOINTS)
    qg, dqg = _step(rc, 1e-3, 1, q, dq, u, np.float64, device_arrays=True, calls=50)
    qr, dqr = ref.steps(q, dq, u, 1e-3, 1, 50)
    eq, edq = rel_err(qg, qr), rel_err(dqg, dqr)
    print(f"plant 50 steps {name}: q {eq:.2e} dq {edq:.2e}")
    assert eq <= TOL_F64 and edq <= TOL_F64


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_gpu_plant_substeps_equal_separate_calls_bitwise(dtype):
    """one call (dt, substeps = 4) == four calls (dt / 4, substeps = 1): dt / 4 is formed once on the host"""
    for name in ("ur5", "jaco2", "ur5_rt"):
        rc, _ = cfg(name)
        q, dq, u = draw(24, 130, rc.N_JOINTS)
        dt = 1e-3
        quarter = dt / 4
        assert quarter * 4 == dt
        a = _step(rc, dt, 4, q, dq, u, dtype, device_arrays=True)
        b = _step(rc, quarter, 1, q, dq, u, dtype, device_arrays=True, calls=4)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_gpu_plant_rows_do_not_depend_on_their_batch_bitwise(dtype):
    for name in ("ur5", "jaco2", "ur5_rt", "gi_synthetic4"):
        rc, _ = cfg(name)
        q, dq, u = draw(25, 130, rc.N_JOINTS)
        full = _step(rc, 1e-3, 4, q, dq, u, dtype) + (_fd(rc, q, dq, u, dtype),)
        for B in BATCHES[:-1]:
            part = _step(rc, 1e-3, 4, q[:B], dq[:B], u[:B], dtype) + (_fd(rc, q[:B], dq[:B], u[:B], dtype),)
            for x, y in zip(part, full):
                assert np.array_equal(x, y[:B]), (name, B)
        perm = np.random.RandomState(26).permutation(130)
        part = _step(rc, 1e-3, 4, q[perm], dq[perm], u[perm], dtype) + (_fd(rc, q[perm], dq[perm], u[perm], dtype),)
        for x, y in zip(part, full):
            assert np.array_equal(x, y[perm]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_gpu_plant_builtin_ur5_equals_compiled_plugin_bitwise(dtype):
    rc, _ = cfg("ur5")
    rp, _ = cfg("ur5_compiled")
    q, dq, u = draw(27, 130, 6)
    assert np.array_equal(_fd(rc, q, dq, u, dtype), _fd(rp, q, dq, u, dtype))
    a, b = _step(rc, 1e-3, 4, q, dq, u, dtype), _step(rp, 1e-3, 4, q, dq, u, dtype)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _closed_loop(B=65):
    import abr_control_amd as a

    rc, _ = cfg("ur5")
    r = np.random.RandomState(28)
    q0 = r.uniform(-1.0, 1.0, (B, 6))
    O = OracleDyn(_abi.load_table("ur5")).O
    tgt = np.zeros((B, 6))
    for b in range(B):
        tgt[b, :3] = O.Tx("EE", q0[b] + 0.2)
    p = _abi.make_osc_params(6, kp=200, use_C=True, use_g=True)
    return a, rc, O, q0, tgt, p


def _ee_dist(O, q, tgt):
    return float(np.mean([np.linalg.norm(O.Tx("EE", q[b]) - tgt[b, :3]) for b in range(q.shape[0])]))


def test_gpu_plant_closed_loop_recorded_plan():
    """OSC (x,y,z, use_C, use_g, kp = 200) followed by plant_step, recorded once into one engine.Plan: launch_graph(30)
    equals 30 eager pairs bit for bit, and after 300 ticks of 1 ms the mean end-effector distance to Tx(EE, q0 + 0.2) is
    below the distance at the start."""
    from abr_control_amd import engine

    a, rc, O, q0, tgt, p = _closed_loop()
    B = q0.shape[0]
    pp = _abi.make_plant_params(1e-3)
    s = a.Stream(0)
    mk = lambda x: a.DeviceArray.from_numpy(np.ascontiguousarray(x))
    # eager pairs
    q_e, dq_e, t_e, u_e = mk(q0), mk(np.zeros((B, 6))), mk(tgt), mk(np.zeros((B, 6)))
    for _ in range(30):
        engine.osc_generate(rc.arm_id, 6, p, q_e, dq_e, t_e, u=u_e, stream=s)
        engine.plant_step(rc.arm_id, 6, pp, q_e, dq_e, u_e, stream=s)
    s.sync()
    # the recorded tick
    q_g, dq_g, t_g, u_g = mk(q0), mk(np.zeros((B, 6))), mk(tgt), mk(np.zeros((B, 6)))
    with engine.Plan(device=0, stream=s) as plan:
        engine.osc_generate(rc.arm_id, 6, p, q_g, dq_g, t_g, u=u_g, stream=s)
        engine.plant_step(rc.arm_id, 6, pp, q_g, dq_g, u_g, stream=s)
    plan.launch_graph(30)
    s.sync()
    for x, y in ((q_e, q_g), (dq_e, dq_g), (u_e, u_g)):
        assert np.array_equal(x.numpy(), y.numpy())
    d0 = _ee_dist(O, q0, tgt)
    plan.launch_graph(270)
    s.sync()
    d1 = _ee_dist(O, q_g.numpy(), tgt)
    print(f"closed loop: mean EE distance {d0:.4f} -> {d1:.4f} m after 300 ticks")
    assert np.isfinite(q_g.numpy()).all() and d1 < d0, (d0, d1)


def test_gpu_plant_singular_inertia_is_reported():
    """a three-joint user table whose last link has neither mass nor inertia: the host-array call raises LinAlgError; the
    device-pointer call reports at the sync of its own stream, not of another (an error code, not a device fault)"""
    import abr_control_amd as a
    from abr_control_amd import arms, engine
    from abr_control_amd._lib import SingularMatrixError

    tab = dict(_abi.load_table("threejoint"))
    tab["name"] = "threejoint_massless_tip"
    tab["mdiag"] = [list(r) for r in tab["mdiag"]]
    tab["mdiag"][3] = [0.0] * 6
    bad = arms.from_table(tab, compiled=False)
    good, _ = cfg("threejoint")
    q, dq, u = draw(29, 65, 3)
    for dtype in DTYPES:
        with pytest.raises(np.linalg.LinAlgError) as ei:
            engine.forward_dynamics(bad.arm_id, 3, q, dq, u, dtype=dtype)
        assert isinstance(ei.value, SingularMatrixError) and ei.value.code == _abi.ESINGULAR
        assert np.isfinite(engine.forward_dynamics(good.arm_id, 3, q, dq, u, dtype=dtype)).all()  # nothing sticks
    sa, sb = a.Stream(0), a.Stream(0)
    qd, dqd, ud = (a.DeviceArray.from_numpy(x) for x in (q, dq, u))
    engine.forward_dynamics(bad.arm_id, 3, qd, dqd, ud, stream=sa)
    ok = engine.forward_dynamics(good.arm_id, 3, qd, dqd, ud, stream=sb)
    sb.sync()  # the healthy stream syncs first: it is not handed the other's flag
    assert np.isfinite(ok.numpy(sb)).all()
    with pytest.raises(np.linalg.LinAlgError):
        sa.sync()
    sa.sync()  # reported once
    engine.plant_step(bad.arm_id, 3, _abi.make_plant_params(1e-3), qd, dqd, ud, stream=sa)
    with pytest.raises(np.linalg.LinAlgError):
        sa.sync()


def test_gpu_arm_sim_is_a_drop_in():
    """the loop of examples/PyGame/force_osc_xy.py:57-78 - ctrlr.generate, then send_forces - 20 times on ur5.Config(),
    one state and B = 64: equal to engine.plant_step called directly"""
    from abr_control_amd import engine
    from abr_control_amd.arms import ArmSim, ur5
    from abr_control_amd.controllers import OSC

    rc = ur5.Config()
    ctrlr = OSC(rc, kp=200, use_C=True)
    pp = _abi.make_plant_params(0.001)
    for shape in ((6,), (64, 6)):
        q0 = np.random.RandomState(30).uniform(-1, 1, shape)
        tgt = np.zeros(shape[:-1] + (6,))
        tgt[..., :3] = [0.3, 0.2, 0.5]
        sim = ArmSim(rc, dt=0.001, q_init=q0)
        sim.connect()
        q, dq = np.array(np.atleast_2d(q0)), np.zeros(np.atleast_2d(q0).shape)
        for _ in range(20):
            fb = sim.get_feedback()
            u = ctrlr.generate(q=fb["q"], dq=fb["dq"], target=tgt)
            assert u.shape == shape
            sim.send_forces(u)
            engine.plant_step(rc.arm_id, 6, pp, q, dq, np.ascontiguousarray(np.atleast_2d(u)))
            assert sim.q.shape == shape and sim.dq.shape == shape
            assert np.array_equal(np.atleast_2d(sim.q), q) and np.array_equal(np.atleast_2d(sim.dq), dq)
        assert abs(sim.t - 0.02) < 1e-12
        assert np.array_equal(rc.forward_dynamics(sim.q, sim.dq, u),
                              engine.forward_dynamics(rc.arm_id, 6, q, dq, np.atleast_2d(u)).reshape(shape))
