"""The plant with non-ideal effects on the GPU (abrk_forward_dynamics_fx_batch, abrk_plant_step_fx_batch, ArmSim) against
the NumPy reference (tests/plant_fx_ref.py), plus the bitwise properties of the kernel and the closed loop with loads as a
recorded plan.  Batches: 1, 63, 64, 65 (either side of a wavefront) and 130 (a partial third wavefront).  A row that the
float64 reference finds within the band of a joint limit (1e-10 fp64, 1e-6 fp32) may decide its bounce the other way and
is left out: none for fp64, at most one per case for fp32, asserted before anything is compared."""
import numpy as np
import pytest

from abr_control_amd import _abi
from tests.plant_fx_ref import ALL_ON, BAND, CAP, TOL_F32, TOL_F64, HostsimGiDyn, OracleDyn, RefFx, draw, \
    effects_rounded, effects_struct, rel_err, rounded

pytestmark = pytest.mark.gpu
BATCHES = (1, 63, 64, 65, 130)
DTYPES = (np.float64, np.float32)


def _config(name):
    """-> (robot_config, reference)"""
    from abr_control_amd import arms
    from tests import compiled_arms, compiled_inertia_arms, compiled_plant_arms

    if name in _abi.BUILTIN_ARMS:
        tab = _abi.load_table(name)
        return getattr(arms, name).Config(), RefFx(OracleDyn(tab), tab)
    if name == "ur5_rt":
        tab = _abi.load_table("ur5")
        return arms.from_table(tab, compiled=False), RefFx(OracleDyn(tab), tab)
    if name == "ur5_compiled":
        tab = compiled_plant_arms.table()
        rc = arms.from_table(tab)
        assert rc.plugin_path, "no ur5_user plugin for the current headers - run build()"
        return rc, RefFx(OracleDyn(tab), tab)
    if name == "synthetic4_compiled":
        tab = compiled_arms.test_arms()["synthetic4"]
        rc = arms.from_table(tab)
        assert rc.plugin_path, "no synthetic4 plugin for the current headers - run build()"
        return rc, RefFx(OracleDyn(tab), tab)
    assert name.startswith("gi_")
    tab = compiled_inertia_arms.table(name[3:])
    ntab = _abi.normalize_table(tab)
    return arms.from_table(tab), RefFx(HostsimGiDyn(ntab), ntab)


_cache = {}


def cfg(name):
    if name not in _cache:
        _cache[name] = _config(name)
    return _cache[name]


def _dev(x, dtype):
    import abr_control_amd as a

    return None if x is None else a.DeviceArray.from_numpy(np.ascontiguousarray(x, dtype=dtype))


def _fd(rc, q, dq, u, dtype, fx=None, ext=None, w=None, device_arrays=False):
    from abr_control_amd import engine

    n = rc.N_JOINTS
    S = effects_struct(n, fx)
    if device_arrays:
        q, dq, u, ext, w = (_dev(x, dtype) for x in (q, dq, u, ext, w))
        return engine.forward_dynamics(rc.arm_id, n, q, dq, u, dtype=dtype, effects=S, tau_ext=ext, wrench=w).numpy()
    return engine.forward_dynamics(rc.arm_id, n, q, dq, u, dtype=dtype, effects=S, tau_ext=ext, wrench=w)


def _step(rc, dt, sub, q, dq, u, dtype, fx=None, ext=None, w=None, device_arrays=False, calls=1, gravity=True,
          after_call=None):
    """`calls` plant steps -> (q, dq) as arrays of `dtype` (the inputs are left alone)"""
    from abr_control_amd import engine

    n = rc.N_JOINTS
    p = _abi.make_plant_params(dt, sub, gravity)
    S = effects_struct(n, fx)
    q, dq, u = (np.array(x, dtype=dtype, order="C") for x in (q, dq, u))
    if device_arrays:
        qd, dqd, ud, ed, wd = (_dev(x, dtype) for x in (q, dq, u, ext, w))
        for _ in range(calls):
            engine.plant_step(rc.arm_id, n, p, qd, dqd, ud, dtype=dtype, effects=S, tau_ext=ed, wrench=wd)
            if after_call is not None:
                after_call(qd.numpy(), dqd.numpy())
        return qd.numpy(), dqd.numpy()
    for _ in range(calls):
        engine.plant_step(rc.arm_id, n, p, q, dq, u, dtype=dtype, effects=S, tau_ext=ext, wrench=w)
        if after_call is not None:
            after_call(q, dq)
    return q, dq


PARITY = ("twojoint", "threejoint", "ur5", "jaco2", "ur5_rt", "ur5_compiled", "synthetic4_compiled", "gi_ur5")
# (effects, tau_ext?, wrench?)
VARIANTS = {"all": (ALL_ON, True, True), "tau_ext": (None, True, False), "wrench": (None, False, True)}
_refs = {}


def _reference(name, variant, dtype):
    """the reference of a parity case at the largest batch, computed once: inputs, ddq, steps per substeps"""
    key = (name, variant, np.dtype(dtype))
    if key not in _refs:
        rc, ref = cfg(name)
        fx, with_ext, with_w = VARIANTS[variant]
        q, dq, u, ext, w = draw(41, BATCHES[-1], rc.N_JOINTS)
        ext, w = (ext if with_ext else None), (w if with_w else None)
        qr, dqr, ur, er, wr = rounded(dtype, q, dq, u, ext, w)
        fxr = effects_rounded(dtype, fx)
        steps = {sub: ref.steps(qr, dqr, ur, 1e-3, sub, 1, fxr, er, wr, band=BAND[np.dtype(dtype)]) for sub in (1, 4)}
        _refs[key] = (q, dq, u, ext, w, ref.ddq(qr, dqr, ur, fxr, er, wr), steps)
    return _refs[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("variant", tuple(VARIANTS))
@pytest.mark.parametrize("name", PARITY)
def test_gpu_plant_fx_parity(name, variant, dtype):
    """ddq and one step (substeps 1 and 4), host arrays and DeviceArrays, every batch size, seed 41"""
    rc, _ = cfg(name)
    dt_ = np.dtype(dtype)
    tol = TOL_F64 if dt_ == np.float64 else TOL_F32
    fx = VARIANTS[variant][0]
    q, dq, u, ext, w, ddq_ref, steps_ref = _reference(name, variant, dtype)
    for sub in (1, 4):
        near = steps_ref[sub][2]
        assert near.sum() <= CAP[dt_], (name, variant, sub, int(near.sum()))
    cut = lambda x, B: None if x is None else x[:B]
    worst = 0.0
    for B in BATCHES:
        for dev in (False, True):
            e = rel_err(_fd(rc, q[:B], dq[:B], u[:B], dtype, fx, cut(ext, B), cut(w, B), dev), ddq_ref[:B])
            worst = max(worst, e)
            assert e <= tol, (name, variant, B, dev, e)
        for sub in (1, 4):
            q1, dq1, near, _ = steps_ref[sub]
            keep = ~near[:B]
            if not keep.any():
                continue
            qg, dqg = _step(rc, 1e-3, sub, q[:B], dq[:B], u[:B], dtype, fx, cut(ext, B), cut(w, B),
                            device_arrays=B % 2 == 0)
            e = max(rel_err(qg[keep], q1[:B][keep]), rel_err(dqg[keep], dq1[:B][keep]))
            worst = max(worst, e)
            assert e <= tol, (name, variant, B, sub, e)
    print(f"plant fx parity {name} {variant} {dt_.name}: worst {worst:.2e}, crossings {steps_ref[1][3]} / "
          f"{steps_ref[4][3]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("ur5", "jaco2"))
def test_gpu_plant_fx_zero_restitution_rests_on_the_limit(name, dtype):
    """restitution = 0, one step at substeps = 1: a crossing joint ends at q == limit and dq == 0 exactly, in the kernel
    and in the reference alike"""
    rc, ref = cfg(name)
    dt_ = np.dtype(dtype)
    tol = TOL_F64 if dt_ == np.float64 else TOL_F32
    fx = dict(ALL_ON, restitution=0.0)
    q, dq, u, ext, w = draw(41, 130, rc.N_JOINTS)
    qr, dqr, ur, er, wr = rounded(dtype, q, dq, u, ext, w)
    q1, dq1, near, crossings = ref.steps(qr, dqr, ur, 1e-3, 1, 1, effects_rounded(dtype, fx), er, wr, band=BAND[dt_])
    assert near.sum() <= CAP[dt_] and crossings >= 15
    keep = ~near
    qg, dqg = _step(rc, 1e-3, 1, q, dq, u, dtype, fx, ext, w)
    hit = (np.abs(q1) == 2.0) & keep[:, None]
    assert hit.sum() >= 15
    assert (qg[hit] == q1[hit]).all() and (dqg[hit] == 0).all() and (dq1[hit] == 0).all()
    assert rel_err(qg[keep], q1[keep]) <= tol and rel_err(dqg[keep], dq1[keep]) <= tol


@pytest.mark.parametrize("name", ("ur5", "jaco2"))
def test_gpu_plant_fx_fifty_steps_and_limits_hold(name):
    """50 calls of 1 ms on DeviceArrays, B = 65, fp64, seed 43, all effects on, against the NumPy loop; after every one
    of the steps q_min <= q <= q_max holds exactly"""
    rc, ref = cfg(name)
    q, dq, u, ext, w = draw(43, 65, rc.N_JOINTS)
    qr, dqr, near, crossings = ref.steps(q, dq, u, 1e-3, 1, 50, ALL_ON, ext, w, band=BAND[np.dtype(np.float64)])
    assert near.sum() == 0
    assert crossings >= 100  # the limits are at work throughout the run
    seen = []

    def inside(qs, dqs):
        seen.append(bool((qs >= -2.0).all() and (qs <= 2.0).all()))

    qg, dqg = _step(rc, 1e-3, 1, q, dq, u, np.float64, ALL_ON, ext, w, device_arrays=True, calls=50, after_call=inside)
    assert len(seen) == 50 and all(seen)
    eq, edq = rel_err(qg, qr), rel_err(dqg, dqr)
    print(f"plant fx 50 steps {name}: q {eq:.2e} dq {edq:.2e} crossings {crossings}")
    assert eq <= TOL_F64 and edq <= TOL_F64


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("ur5", "jaco2", "ur5_rt", "gi_ur5"))
def test_gpu_plant_fx_everything_off_equals_the_plain_kernel_bitwise(name, dtype):
    """an effects struct without flags, zero arrays on top of it, a zero tau_ext alone: the bits of
    abrk_plant_step_batch / abrk_forward_dynamics_batch.
    The dynamics pass of the two kernels has to leave the compiler identical for this (abrk_ctrl.h plant_fx_row says what
    that takes): with the tau phase reading sin / cos and dq in front of the pass, jaco2 and ur5_rt were one unit in the
    last place off on 1 - 2 of 780 values."""
    rc, _ = cfg(name)
    n = rc.N_JOINTS
    q, dq, u, _, _ = draw(44, 130, n)
    plain = _step(rc, 1e-3, 4, q, dq, u, dtype) + (_fd(rc, q, dq, u, dtype),)
    zn, z6 = np.zeros((130, n)), np.zeros((130, 6))
    worst = 0.0
    for fx, ext, w in (({}, None, None), ({}, zn, z6), (None, zn, None)):
        got = _step(rc, 1e-3, 4, q, dq, u, dtype, fx, ext, w) + (_fd(rc, q, dq, u, dtype, fx, ext, w),)
        for what, x, y in zip(("q", "dq", "ddq"), got, plain):
            d = float(np.max(np.abs(x.astype(np.float64) - y.astype(np.float64))))
            worst = max(worst, d)
            print(f"everything off {name} {np.dtype(dtype).name} ext={ext is not None} w={w is not None} {what}: "
                  f"max|d| {d:.3e}, {int((x != y).sum())} of {x.size} values differ")
    assert worst == 0.0, (name, worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_gpu_plant_fx_substeps_equal_separate_calls_bitwise(dtype):
    """one call (dt, substeps = 4) == four calls (dt / 4, substeps = 1), limits and bounces included"""
    for name in ("ur5", "jaco2", "ur5_rt"):
        rc, _ = cfg(name)
        q, dq, u, ext, w = draw(41, 130, rc.N_JOINTS)
        dt = 1e-3
        quarter = dt / 4
        assert quarter * 4 == dt
        a = _step(rc, dt, 4, q, dq, u, dtype, ALL_ON, ext, w, device_arrays=True)
        b = _step(rc, quarter, 1, q, dq, u, dtype, ALL_ON, ext, w, device_arrays=True, calls=4)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_gpu_plant_fx_rows_do_not_depend_on_their_batch_bitwise(dtype):
    for name in ("ur5", "jaco2", "ur5_rt", "gi_ur5"):
        rc, _ = cfg(name)
        q, dq, u, ext, w = draw(41, 130, rc.N_JOINTS)
        run = lambda s: _step(rc, 1e-3, 4, q[s], dq[s], u[s], dtype, ALL_ON, ext[s], w[s]) + (
            _fd(rc, q[s], dq[s], u[s], dtype, ALL_ON, ext[s], w[s]),)
        full = run(slice(None))
        for B in BATCHES[:-1]:
            for x, y in zip(run(slice(0, B)), full):
                assert np.array_equal(x, y[:B]), (name, B)
        perm = np.random.RandomState(26).permutation(130)
        for x, y in zip(run(perm), full):
            assert np.array_equal(x, y[perm]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_gpu_plant_fx_builtin_ur5_equals_compiled_plugin_bitwise(dtype):
    rc, _ = cfg("ur5")
    rp, _ = cfg("ur5_compiled")
    q, dq, u, ext, w = draw(41, 130, 6)
    assert np.array_equal(_fd(rc, q, dq, u, dtype, ALL_ON, ext, w), _fd(rp, q, dq, u, dtype, ALL_ON, ext, w))
    a, b = _step(rc, 1e-3, 4, q, dq, u, dtype, ALL_ON, ext, w), _step(rp, 1e-3, 4, q, dq, u, dtype, ALL_ON, ext, w)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", ("ur5", "twojoint"))
def test_gpu_plant_fx_viscous_friction_dissipates(name):
    """u = 0, gravity off, viscous 0.5 only, 200 steps of 1 ms, B = 65, fp64: the kinetic energy dq^T M dq / 2 (M from
    the oracle) is lower than at the start on every row.  The reference gives at most 0.986 (twojoint) and 0.957 (ur5) of
    the start."""
    rc, ref = cfg(name)
    n = rc.N_JOINTS
    r = np.random.RandomState(45)
    q = r.uniform(-np.pi, np.pi, (65, n))
    dq = r.uniform(-2, 2, (65, n))
    ke = lambda qs, dqs: np.array([0.5 * dqs[b] @ ref.O.M(qs[b]) @ dqs[b] for b in range(qs.shape[0])])
    e0 = ke(q, dq)
    qg, dqg = _step(rc, 1e-3, 1, q, dq, np.zeros((65, n)), np.float64, dict(damping=0.5), device_arrays=True, calls=200,
                    gravity=False)
    ratio = ke(qg, dqg) / e0
    print(f"dissipation {name}: kinetic energy at most {ratio.max():.4f} of the start")
    assert np.isfinite(ratio).all() and (ratio < 1.0).all(), ratio.max()


def test_gpu_plant_fx_closed_loop_recorded_plan():
    """{ osc_generate (kp = 200, use_C, use_g); plant_step with effects, tau_ext and wrench } for 65 UR5 arms, recorded
    once: launch_graph(30) equals 30 eager pairs bit for bit; after the wrench array is overwritten on the plan's stream,
    30 more ticks equal an eager run that made the same change"""
    import abr_control_amd as a
    from abr_control_amd import engine

    rc, ref = cfg("ur5")
    B = 65
    r = np.random.RandomState(46)
    q0 = r.uniform(-1.0, 1.0, (B, 6))
    tgt = np.zeros((B, 6))
    for b in range(B):
        tgt[b, :3] = ref.O.Tx("EE", q0[b] + 0.2)
    ext0 = r.uniform(-1, 1, (B, 6))
    w0 = r.uniform(-5, 5, (B, 6))
    w1 = r.uniform(-20, 20, (B, 6))
    p = _abi.make_osc_params(6, kp=200, use_C=True, use_g=True)
    pp = _abi.make_plant_params(1e-3, 2)
    S = effects_struct(6, ALL_ON)
    s = a.Stream(0)
    mk = lambda x: a.DeviceArray.from_numpy(np.ascontiguousarray(x))

    def tick(q, dq, t, u, e, w):
        engine.osc_generate(rc.arm_id, 6, p, q, dq, t, u=u, stream=s)
        engine.plant_step(rc.arm_id, 6, pp, q, dq, u, stream=s, effects=S, tau_ext=e, wrench=w)

    eager = [mk(q0), mk(np.zeros((B, 6))), mk(tgt), mk(np.zeros((B, 6))), mk(ext0), mk(w0)]
    graph = [mk(q0), mk(np.zeros((B, 6))), mk(tgt), mk(np.zeros((B, 6))), mk(ext0), mk(w0)]
    with engine.Plan(device=0, stream=s) as plan:
        tick(*graph)
    for wrench in (None, w1):
        if wrench is not None:
            for arrs in (eager, graph):
                arrs[5].copy_from_numpy(wrench, stream=s)
        for _ in range(30):
            tick(*eager)
        plan.launch_graph(30)
        s.sync()
        for x, y in zip(eager[:4], graph[:4]):
            assert np.array_equal(x.numpy(), y.numpy())
        assert np.isfinite(graph[0].numpy()).all()
    # the new wrench did reach the plan: a run that kept the old one ends elsewhere
    kept = [mk(q0), mk(np.zeros((B, 6))), mk(tgt), mk(np.zeros((B, 6))), mk(ext0), mk(w0)]
    for _ in range(60):
        tick(*kept)
    s.sync()
    assert not np.array_equal(kept[0].numpy(), graph[0].numpy())


def test_gpu_plant_fx_arm_sim_equals_engine():
    """ArmSim with effects, tau_ext and wrench: equal to engine.plant_step with the same arguments, one state and B = 64"""
    from abr_control_amd import engine
    from abr_control_amd.arms import ArmSim, ur5

    rc = ur5.Config()
    S = effects_struct(6, ALL_ON)
    pp = _abi.make_plant_params(0.001, 2)
    r = np.random.RandomState(47)
    for shape in ((6,), (64, 6)):
        q0 = r.uniform(-1.9, 1.9, shape)
        sim = ArmSim(rc, dt=0.001, q_init=q0, substeps=2, effects=S)
        sim.connect()
        q, dq = np.array(np.atleast_2d(q0)), np.zeros(np.atleast_2d(q0).shape)
        for _ in range(10):
            u = r.uniform(-20, 20, shape)
            ext = r.uniform(-5, 5, shape)
            w = r.uniform(-10, 10, shape[:-1] + (6,))
            sim.send_forces(u, tau_ext=ext, wrench=w)
            engine.plant_step(rc.arm_id, 6, pp, q, dq, np.atleast_2d(u), effects=S, tau_ext=np.atleast_2d(ext),
                              wrench=np.atleast_2d(w))
            assert sim.q.shape == shape and sim.dq.shape == shape
            assert np.array_equal(np.atleast_2d(sim.q), q) and np.array_equal(np.atleast_2d(sim.dq), dq)
        # a wrench shared by every arm broadcasts
        sim.send_forces(u, wrench=w.reshape(-1, 6)[0])
        engine.plant_step(rc.arm_id, 6, pp, q, dq, np.atleast_2d(u), effects=S,
                          wrench=np.ascontiguousarray(np.broadcast_to(w.reshape(-1, 6)[0], (q.shape[0], 6))))
        assert np.array_equal(np.atleast_2d(sim.q), q)


def test_gpu_plant_fx_mixing_host_and_device_arrays_is_refused():
    import abr_control_amd as a
    from abr_control_amd import engine

    rc, _ = cfg("ur5")
    q, dq, u, ext, w = draw(48, 4, 6)
    qd, dqd, ud = (a.DeviceArray.from_numpy(x) for x in (q, dq, u))
    with pytest.raises(TypeError, match="mixing DeviceArray and NumPy"):
        engine.plant_step(rc.arm_id, 6, _abi.make_plant_params(1e-3), qd, dqd, ud, wrench=w)
    with pytest.raises(TypeError, match="mixing DeviceArray and NumPy"):
        engine.forward_dynamics(rc.arm_id, 6, q, dq, u, tau_ext=a.DeviceArray.from_numpy(ext))


def test_gpu_plant_fx_singular_inertia_is_reported():
    """a three-joint user table whose last link has neither mass nor inertia, through the new entry points: the
    host-array call raises LinAlgError; the device-pointer call reports at the sync of its own stream, not of another"""
    import abr_control_amd as a
    from abr_control_amd import arms, engine
    from abr_control_amd._lib import SingularMatrixError

    tab = dict(_abi.load_table("threejoint"))
    tab["name"] = "threejoint_massless_tip"
    tab["mdiag"] = [list(r) for r in tab["mdiag"]]
    tab["mdiag"][3] = [0.0] * 6
    bad = arms.from_table(tab, compiled=False)
    good, _ = cfg("threejoint")
    q, dq, u, ext, w = draw(49, 65, 3)
    S = effects_struct(3, ALL_ON)
    for dtype in DTYPES:
        with pytest.raises(np.linalg.LinAlgError) as ei:
            engine.forward_dynamics(bad.arm_id, 3, q, dq, u, dtype=dtype, effects=S, tau_ext=ext, wrench=w)
        assert isinstance(ei.value, SingularMatrixError) and ei.value.code == _abi.ESINGULAR
        ok = engine.forward_dynamics(good.arm_id, 3, q, dq, u, dtype=dtype, effects=S, tau_ext=ext, wrench=w)
        assert np.isfinite(ok).all()  # nothing sticks
    sa, sb = a.Stream(0), a.Stream(0)
    qd, dqd, ud, ed, wd = (a.DeviceArray.from_numpy(x) for x in (q, dq, u, ext, w))
    engine.forward_dynamics(bad.arm_id, 3, qd, dqd, ud, stream=sa, effects=S, tau_ext=ed, wrench=wd)
    ok = engine.forward_dynamics(good.arm_id, 3, qd, dqd, ud, stream=sb, effects=S, tau_ext=ed, wrench=wd)
    sb.sync()  # the healthy stream syncs first: it is not handed the other's flag
    assert np.isfinite(ok.numpy(sb)).all()
    with pytest.raises(np.linalg.LinAlgError):
        sa.sync()
    sa.sync()  # reported once
    engine.plant_step(bad.arm_id, 3, _abi.make_plant_params(1e-3), qd, dqd, ud, stream=sa, effects=S, wrench=wd)
    with pytest.raises(np.linalg.LinAlgError):
        sa.sync()
