"""The plant with a payload at the end effector on the GPU (abrk_forward_dynamics_payload_batch,
abrk_plant_step_payload_batch, ArmSim(payload=...)) against the NumPy reference (tests/plant_payload_ref.py), the
augmented-table identity, the bitwise properties of the kernel and a recorded closed loop whose payload array is rewritten
between replays.  Batches: 1, 63, 64, 65 (either side of a wavefront) and 130 (a partial third wavefront).  States and
loads: seed 41; payloads: seed 43 (m in 0.2 - 3 kg, r within 10 cm, every seventh row m = 0).  Bars: 1e-6 (fp64) and 1e-4
(fp32) on max|d| / max|ref| per row.  With the limits on, a row that the float64 reference finds within the band of a
limit is left out (none occur; the caps of the effects tests are asserted before anything is compared)."""
import copy
import ctypes as C

import numpy as np
import pytest

from abr_control_amd import _abi, plant_payload
from tests.plant_payload_ref import ALL_ON, BAND, CAP, SEED, SEED_PAYLOAD, TOL_F32, TOL_F64, HostsimGiDyn, OracleDyn, \
    RefPayload, draw, draw_payload, effects_rounded, effects_struct, rel_err, rounded

pytestmark = pytest.mark.gpu
BATCHES = (1, 63, 64, 65, 130)
DTYPES = (np.float64, np.float32)


def tol_of(dtype):
    return TOL_F64 if np.dtype(dtype) == np.float64 else TOL_F32


def _config(name):
    """-> (robot_config, reference)"""
    from abr_control_amd import arms
    from tests import compiled_arms, compiled_inertia_arms, compiled_plant_arms

    if name in _abi.BUILTIN_ARMS:
        tab = _abi.load_table(name)
        return getattr(arms, name).Config(), RefPayload(OracleDyn(tab), tab)
    if name == "ur5_rt":
        tab = _abi.load_table("ur5")
        return arms.from_table(tab, compiled=False), RefPayload(OracleDyn(tab), tab)
    if name == "ur5_compiled":
        tab = compiled_plant_arms.table()
        rc = arms.from_table(tab)
        assert rc.plugin_path, "no ur5_user plugin for the current headers - run build()"
        return rc, RefPayload(OracleDyn(tab), tab)
    if name == "synthetic4_compiled":
        tab = compiled_arms.test_arms()["synthetic4"]
        rc = arms.from_table(tab)
        assert rc.plugin_path, "no synthetic4 plugin for the current headers - run build()"
        return rc, RefPayload(OracleDyn(tab), tab)
    assert name.startswith("gi_")
    tab = compiled_inertia_arms.table(name[3:])
    ntab = _abi.normalize_table(tab)
    return arms.from_table(tab), RefPayload(HostsimGiDyn(ntab), ntab)


_cache = {}


def cfg(name):
    if name not in _cache:
        _cache[name] = _config(name)
    return _cache[name]


def _dev(x, dtype):
    import abr_control_amd as a

    return None if x is None else a.DeviceArray.from_numpy(np.ascontiguousarray(x, dtype=dtype))


def _host(x, dtype):
    return None if x is None else np.ascontiguousarray(x, dtype=dtype)


def _fd(rc, q, dq, u, p, dtype, fx=None, ext=None, w=None, device_arrays=False):
    from abr_control_amd import engine

    n = rc.N_JOINTS
    S = effects_struct(n, fx)
    conv = _dev if device_arrays else _host
    q, dq, u, ext, w, p = (conv(x, dtype) for x in (q, dq, u, ext, w, p))
    out = plant_payload.forward_dynamics(rc.arm_id, n, q, dq, u, dtype=dtype, effects=S, tau_ext=ext, wrench=w,
                                         payload=p)
    return out.numpy() if device_arrays else out


def _step(rc, dt, sub, q, dq, u, p, dtype, fx=None, ext=None, w=None, device_arrays=False, calls=1, after_call=None):
    """`calls` plant steps -> (q, dq) as arrays of `dtype` (the inputs are left alone)"""
    from abr_control_amd import engine

    n = rc.N_JOINTS
    pp = _abi.make_plant_params(dt, sub, True)
    S = effects_struct(n, fx)
    q, dq = (np.array(x, dtype=dtype, order="C") for x in (q, dq))
    conv = _dev if device_arrays else _host
    qd, dqd, ud, ed, wd, pd = (conv(x, dtype) for x in (q, dq, u, ext, w, p))
    for _ in range(calls):
        plant_payload.plant_step(rc.arm_id, n, pp, qd, dqd, ud, dtype=dtype, effects=S, tau_ext=ed, wrench=wd,
                                 payload=pd)
        if after_call is not None:
            after_call(qd.numpy() if device_arrays else qd, dqd.numpy() if device_arrays else dqd)
    return (qd.numpy(), dqd.numpy()) if device_arrays else (qd, dqd)


PARITY = ("twojoint", "threejoint", "ur5", "jaco2", "ur5_rt", "ur5_compiled", "synthetic4_compiled", "gi_ur5")
# (effects, tau_ext and wrench?)
VARIANTS = {"payload": (None, False), "all": (ALL_ON, True)}
_refs = {}


def _reference(name, variant, dtype):
    """the reference of a parity case at the largest batch, computed once: inputs, ddq, steps per substeps"""
    key = (name, variant, np.dtype(dtype))
    if key not in _refs:
        rc, ref = cfg(name)
        fx, loads = VARIANTS[variant]
        q, dq, u, ext, w = draw(SEED, BATCHES[-1], rc.N_JOINTS)
        if not loads:
            ext = w = None
        p = draw_payload(SEED_PAYLOAD, BATCHES[-1])
        qr, dqr, ur, er, wr, pr = rounded(dtype, q, dq, u, ext, w, p)
        fxr = effects_rounded(dtype, fx)
        ref.set_payload(pr)
        steps = {sub: ref.steps(qr, dqr, ur, 1e-3, sub, 1, fxr, er, wr, band=BAND[np.dtype(dtype)]) for sub in (1, 4)}
        _refs[key] = (q, dq, u, ext, w, p, ref.ddq(qr, dqr, ur, fxr, er, wr), steps)
    return _refs[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("variant", tuple(VARIANTS))
@pytest.mark.parametrize("name", PARITY)
def test_gpu_plant_payload_parity(name, variant, dtype):
    """ddq and one step (substeps 1 and 4), host arrays and DeviceArrays, every batch size"""
    rc, _ = cfg(name)
    dt_ = np.dtype(dtype)
    tol = tol_of(dtype)
    fx = VARIANTS[variant][0]
    q, dq, u, ext, w, p, ddq_ref, steps_ref = _reference(name, variant, dtype)
    for sub in (1, 4):
        near = steps_ref[sub][2]
        assert near.sum() <= CAP[dt_], (name, variant, sub, int(near.sum()))
    cut = lambda x, B: None if x is None else x[:B]
    worst = 0.0
    for B in BATCHES:
        for dev in (False, True):
            e = rel_err(_fd(rc, q[:B], dq[:B], u[:B], p[:B], dtype, fx, cut(ext, B), cut(w, B), dev), ddq_ref[:B])
            worst = max(worst, e)
            assert e <= tol, (name, variant, B, dev, e)
        for sub in (1, 4):
            q1, dq1, near, _ = steps_ref[sub]
            keep = ~near[:B]
            if not keep.any():
                continue
            qg, dqg = _step(rc, 1e-3, sub, q[:B], dq[:B], u[:B], p[:B], dtype, fx, cut(ext, B), cut(w, B),
                            device_arrays=B % 2 == 0)
            e = max(rel_err(qg[keep], q1[:B][keep]), rel_err(dqg[keep], dq1[:B][keep]))
            worst = max(worst, e)
            assert e <= tol, (name, variant, B, sub, e)
    print(f"plant payload parity {name} {variant} {dt_.name}: worst {worst:.2e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("ur5", "twojoint", "threejoint"))
def test_gpu_plant_payload_is_the_arm_with_a_heavier_last_link(name, dtype):
    """m = 1.7 kg on every row at the last link's centre of mass, B = 130: the payload entry on the built-in arm and on
    the runtime-table arm against the PLAIN entry on the table whose mdiag[-1][0:3] is raised by m (runtime table)"""
    from abr_control_amd import arms, engine
    from oracle.oracle import Oracle

    tab = _abi.load_table(name)
    n = int(tab["n_joints"])
    O = Oracle(tab)
    q, dq, u, _, _ = draw(SEED, 130, n)
    r = O.R("EE", q[0]).T @ (O.Tx(f"link{n}", q[0]) - O.Tx("EE", q[0]))
    m = 1.7
    p = np.tile(np.concatenate([[m], r]), (130, 1))
    aug = copy.deepcopy(tab)
    aug["name"] = f"{name}_plus_payload"
    aug["mdiag"] = [list(map(float, row)) for row in aug["mdiag"]]
    for k in range(3):
        aug["mdiag"][-1][k] += m
    heavy = arms.from_table(aug, compiled=False)
    tol = tol_of(dtype)
    cast = lambda x: np.ascontiguousarray(x, dtype=dtype)
    want = engine.forward_dynamics(heavy.arm_id, n, cast(q), cast(dq), cast(u), dtype=dtype)
    bare = engine.forward_dynamics(cfg(name)[0].arm_id, n, cast(q), cast(dq), cast(u), dtype=dtype)
    assert rel_err(bare, want) > 0.05  # the mass matters
    qa, dqa = cast(q).copy(), cast(dq).copy()
    engine.plant_step(heavy.arm_id, n, _abi.make_plant_params(1e-3, 4), qa, dqa, cast(u), dtype=dtype)
    for rc in (cfg(name)[0], arms.from_table(tab, compiled=False)):
        e = rel_err(_fd(rc, q, dq, u, p, dtype), want)
        qg, dqg = _step(rc, 1e-3, 4, q, dq, u, p, dtype)
        eq, edq = rel_err(qg, qa), rel_err(dqg, dqa)
        print(f"augmented table {name} {np.dtype(dtype).name}: ddq {e:.2e} q {eq:.2e} dq {edq:.2e}")
        assert e <= tol and eq <= tol and edq <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_gpu_plant_payload_substeps_equal_separate_calls_bitwise(dtype):
    """one call (dt, substeps = 4) == four calls (dt / 4, substeps = 1), limits and bounces included"""
    for name in ("ur5", "jaco2", "ur5_rt"):
        rc, _ = cfg(name)
        q, dq, u, ext, w = draw(SEED, 130, rc.N_JOINTS)
        p = draw_payload(SEED_PAYLOAD, 130)
        dt = 1e-3
        quarter = dt / 4
        assert quarter * 4 == dt
        a = _step(rc, dt, 4, q, dq, u, p, dtype, ALL_ON, ext, w, device_arrays=True)
        b = _step(rc, quarter, 1, q, dq, u, p, dtype, ALL_ON, ext, w, device_arrays=True, calls=4)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_gpu_plant_payload_rows_do_not_depend_on_their_batch_bitwise(dtype):
    """rows of B = 130 against the same rows run at B = 1 and 65 (and the other batch sizes)"""
    for name in ("ur5", "jaco2", "ur5_rt", "gi_ur5"):
        rc, _ = cfg(name)
        q, dq, u, ext, w = draw(SEED, 130, rc.N_JOINTS)
        p = draw_payload(SEED_PAYLOAD, 130)
        run = lambda s: _step(rc, 1e-3, 4, q[s], dq[s], u[s], p[s], dtype, ALL_ON, ext[s], w[s]) + (
            _fd(rc, q[s], dq[s], u[s], p[s], dtype, ALL_ON, ext[s], w[s]),)
        full = run(slice(None))
        for B in BATCHES[:-1]:
            for x, y in zip(run(slice(0, B)), full):
                assert np.array_equal(x, y[:B]), (name, B)
        for x, y in zip(run(slice(70, 71)), full):  # a row of the second wavefront, alone
            assert np.array_equal(x, y[70:71]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_gpu_plant_payload_builtin_ur5_equals_compiled_plugin_bitwise(dtype):
    rc, _ = cfg("ur5")
    rp, _ = cfg("ur5_compiled")
    q, dq, u, ext, w = draw(SEED, 130, 6)
    p = draw_payload(SEED_PAYLOAD, 130)
    assert np.array_equal(_fd(rc, q, dq, u, p, dtype, ALL_ON, ext, w), _fd(rp, q, dq, u, p, dtype, ALL_ON, ext, w))
    a = _step(rc, 1e-3, 4, q, dq, u, p, dtype, ALL_ON, ext, w)
    b = _step(rp, 1e-3, 4, q, dq, u, p, dtype, ALL_ON, ext, w)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("ur5", "jaco2", "ur5_rt"))
def test_gpu_plant_payload_null_is_the_effects_entry_bitwise_and_zero_mass_is_close(name, dtype):
    """the C entries with payload == NULL: the bits of the *_fx entries; m = 0 on every row: within the bar of them"""
    from abr_control_amd import engine
    from abr_control_amd._lib import check, lib

    rc, _ = cfg(name)
    n = rc.N_JOINTS
    B = 130
    q, dq, u, ext, w = (np.ascontiguousarray(x, dtype=dtype) for x in draw(SEED, B, n))
    S = effects_struct(n, ALL_ON)
    pp = _abi.make_plant_params(1e-3, 4)
    code = 0 if np.dtype(dtype) == np.float64 else 1
    vp = lambda a: C.c_void_p(a.ctypes.data)
    want_ddq = engine.forward_dynamics(rc.arm_id, n, q, dq, u, dtype=dtype, effects=S, tau_ext=ext, wrench=w)
    got_ddq = np.full_like(q, np.nan)
    check(lib().abrk_forward_dynamics_payload_batch(rc.arm_id, code, C.byref(S), B, vp(q), vp(dq), vp(u), vp(ext),
                                                    vp(w), None, vp(got_ddq), 0, None))
    assert np.array_equal(got_ddq, want_ddq)
    qa, dqa, qb, dqb = q.copy(), dq.copy(), q.copy(), dq.copy()
    engine.plant_step(rc.arm_id, n, pp, qa, dqa, u, dtype=dtype, effects=S, tau_ext=ext, wrench=w)
    check(lib().abrk_plant_step_payload_batch(rc.arm_id, code, C.byref(pp), C.byref(S), B, vp(qb), vp(dqb), vp(u),
                                              vp(ext), vp(w), None, 0, None))
    assert np.array_equal(qa, qb) and np.array_equal(dqa, dqb)
    # m = 0 (with an offset all the same): the neutral value
    p0 = draw_payload(SEED_PAYLOAD, B)
    p0[:, 0] = 0
    tol = tol_of(dtype)
    assert rel_err(_fd(rc, q, dq, u, p0, dtype, ALL_ON, ext, w), want_ddq) <= tol
    qg, dqg = _step(rc, 1e-3, 4, q, dq, u, p0, dtype, ALL_ON, ext, w)
    assert rel_err(qg, qa) <= tol and rel_err(dqg, dqa) <= tol


@pytest.mark.parametrize("name", ("ur5", "jaco2"))
def test_gpu_plant_payload_fifty_steps_and_limits_hold(name):
    """50 calls of 1 ms on DeviceArrays, B = 65, fp64, everything on, against the NumPy loop; after every one of the
    steps q_min <= q <= q_max holds exactly"""
    rc, ref = cfg(name)
    q, dq, u, ext, w = draw(SEED_PAYLOAD, 65, rc.N_JOINTS)
    p = draw_payload(SEED_PAYLOAD, 65)
    qr, dqr, near, crossings = ref.set_payload(p).steps(q, dq, u, 1e-3, 1, 50, ALL_ON, ext, w,
                                                        band=BAND[np.dtype(np.float64)])
    assert near.sum() == 0
    assert crossings >= 100  # (the reference counts 128 on ur5, 195 on jaco2) the limits are at work throughout the run
    seen = []

    def inside(qs, dqs):
        seen.append(bool((qs >= -2.0).all() and (qs <= 2.0).all()))

    qg, dqg = _step(rc, 1e-3, 1, q, dq, u, p, np.float64, ALL_ON, ext, w, device_arrays=True, calls=50,
                    after_call=inside)
    assert len(seen) == 50 and all(seen)
    eq, edq = rel_err(qg, qr), rel_err(dqg, dqr)
    print(f"plant payload 50 steps {name}: q {eq:.2e} dq {edq:.2e} crossings {crossings}")
    assert eq <= TOL_F64 and edq <= TOL_F64


def test_gpu_plant_payload_recorded_plan_picks_up_a_rewritten_mass():
    """{ osc_generate (kp = 200, use_C); plant_step(payload = p) } for 64 UR5 arms, recorded once: launch_graph(20), every
    mass doubled in p, launch_graph(20) - equal, bit for bit, to the same 40 ticks issued as separate calls with the
    rewrite at tick 20; and different from a run that kept the first masses"""
    import abr_control_amd as a
    from abr_control_amd import engine

    rc, ref = cfg("ur5")
    B = 64
    r = np.random.RandomState(46)
    q0 = r.uniform(-1.0, 1.0, (B, 6))
    tgt = np.zeros((B, 6))
    for b in range(B):
        tgt[b, :3] = ref.O.Tx("EE", q0[b] + 0.2)
    p0 = draw_payload(SEED_PAYLOAD, B)
    p1 = p0.copy()
    p1[:, 0] *= 2
    op = _abi.make_osc_params(6, kp=200, use_C=True)
    pp = _abi.make_plant_params(1e-3, 2)
    s = a.Stream(0)
    mk = lambda x: a.DeviceArray.from_numpy(np.ascontiguousarray(x))

    def tick(q, dq, t, u, p):
        engine.osc_generate(rc.arm_id, 6, op, q, dq, t, u=u, stream=s)
        plant_payload.plant_step(rc.arm_id, 6, pp, q, dq, u, stream=s, payload=p)

    fresh = lambda: [mk(q0), mk(np.zeros((B, 6))), mk(tgt), mk(np.zeros((B, 6))), mk(p0)]
    eager, graph, kept = fresh(), fresh(), fresh()
    with engine.Plan(device=0, stream=s) as plan:
        tick(*graph)
    for payload in (None, p1):
        if payload is not None:
            for arrs in (eager, graph):
                arrs[4].copy_from_numpy(payload, stream=s)
        for _ in range(20):
            tick(*eager)
        plan.launch_graph(20)
        s.sync()
        for x, y in zip(eager[:4], graph[:4]):
            assert np.array_equal(x.numpy(), y.numpy())
        assert np.isfinite(graph[0].numpy()).all()
    for _ in range(40):
        tick(*kept)
    s.sync()
    assert not np.array_equal(kept[0].numpy(), graph[0].numpy())


def test_gpu_plant_payload_arm_sim_equals_engine():
    """ArmSim(payload=...) - one payload for one arm, one for all of B = 64, one per arm - equals engine.plant_step"""
    from abr_control_amd import engine
    from abr_control_amd.arms import ArmSim, ur5

    rc = ur5.Config()
    pp = _abi.make_plant_params(0.001, 2)
    r = np.random.RandomState(47)
    rows = draw_payload(SEED_PAYLOAD, 64)
    for shape, payload in (((6,), (1.5, [0.0, 0.02, 0.1])), ((64, 6), (1.5, [0.0, 0.02, 0.1])), ((64, 6), rows)):
        q0 = r.uniform(-1.9, 1.9, shape)
        sim = ArmSim(rc, dt=0.001, q_init=q0, substeps=2, payload=payload)
        sim.connect()
        q, dq = np.array(np.atleast_2d(q0)), np.zeros(np.atleast_2d(q0).shape)
        p = rows if payload is rows else np.tile([1.5, 0.0, 0.02, 0.1], (q.shape[0], 1))
        for _ in range(5):
            u = r.uniform(-20, 20, shape)
            sim.send_forces(u)
            plant_payload.plant_step(rc.arm_id, 6, pp, q, dq, np.atleast_2d(u), payload=p)
            assert sim.q.shape == shape and sim.dq.shape == shape
            assert np.array_equal(np.atleast_2d(sim.q), q) and np.array_equal(np.atleast_2d(sim.dq), dq)
    # set_payload: another mass from the next step on
    sim.set_payload((0.5, [0.0, 0.0, 0.0]))
    sim.send_forces(u)
    plant_payload.plant_step(rc.arm_id, 6, pp, q, dq, np.atleast_2d(u), payload=np.tile([0.5, 0.0, 0.0, 0.0], (64, 1)))
    assert np.array_equal(np.atleast_2d(sim.q), q) and np.array_equal(np.atleast_2d(sim.dq), dq)


def test_gpu_plant_payload_mixing_host_and_device_arrays_is_refused():
    import abr_control_amd as a
    from abr_control_amd import engine

    rc, _ = cfg("ur5")
    q, dq, u, _, _ = draw(48, 4, 6)
    p = draw_payload(SEED_PAYLOAD, 4)
    qd, dqd, ud = (a.DeviceArray.from_numpy(x) for x in (q, dq, u))
    with pytest.raises(TypeError, match="mixing DeviceArray and NumPy"):
        plant_payload.plant_step(rc.arm_id, 6, _abi.make_plant_params(1e-3), qd, dqd, ud, payload=p)
    with pytest.raises(TypeError, match="mixing DeviceArray and NumPy"):
        plant_payload.forward_dynamics(rc.arm_id, 6, q, dq, u, payload=a.DeviceArray.from_numpy(p))
