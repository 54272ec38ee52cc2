"""InverseKinematics.generate_path on the device (abrk_ik_generate_path_batch, ik_kernel): every arm family and joint
count, float64 and float32, the three methods, against the C oracle one step at a time (cases, gates, the cap on what is
left out and the bar: tests/ik_cases.py, proven on the host build by tests/test_ik_hostsim.py); whole paths teacher-forced;
the properties that hold on every row; the Cholesky path of pinv_KxN against its Jacobi fallback; rows independent of
their batch, of where their arrays live and of the kernel family, bit for bit; convergence; the class.
Figures observed on an MI355X: profiles/ik_tests.md."""
import ctypes as C
import functools

import numpy as np
import pytest

from abr_control_amd import _abi
from tests import ik_cases as K

pytestmark = pytest.mark.gpu

BUILTIN = ("onejoint", "twojoint", "threejoint", "ur5", "jaco2")
STEP_ARMS = BUILTIN + ("ur5_rt",) + tuple(f"synth{n}" for n in range(1, 8)) + ("ur5_compiled", "synthetic4_compiled")
PATH_ARMS = ("ur5", "jaco2", "threejoint", "twojoint", "synth7")
DTYPES = pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
METHODS = pytest.mark.parametrize("method", (1, 2, 3))


@functools.lru_cache(maxsize=None)
def _backend(arm_id):
    """static kernels for the built-ins, the runtime-table kernels for the tables, the plugin for *_compiled"""
    from tests import cases

    if arm_id in BUILTIN:
        return cases.GpuBackend(arm_id)
    return cases.GpuBackend(K.arm_table(arm_id), "compiled" if arm_id.endswith("_compiled") else "rt")


def _call(arm_id, p, q, tgt, dtype, **kw):
    from abr_control_amd import engine

    be = _backend(arm_id)
    return engine.ik_generate_path(be.arm_id, be.n, p, q, tgt, dtype=dtype, **kw)


def _run(arm_id, dtype):
    return lambda p, q, tgt: _call(arm_id, p, q, tgt, dtype)


# ---------------------------------------------------------------- (a) one step, every arm family
@METHODS
@DTYPES
@pytest.mark.parametrize("arm_id", STEP_ARMS)
def test_gpu_ik_one_step_every_arm(arm_id, dtype, method):
    """130 rows - two wavefronts and a ragged third - of one step under the three limit sets: the singular block, the
    random rows and the near-target rows in one call; every clamp seen engaged and not engaged on the reference"""
    clamps = K.Clamps()
    K.run_one_step(_run(arm_id, dtype), arm_id, dtype, method, 130, K.SEED_STEP, clamps)
    clamps.check(f"{arm_id} method {method}")


# ---------------------------------------------------------------- (b) whole paths
@METHODS
@DTYPES
@pytest.mark.parametrize("arm_id", PATH_ARMS)
def test_gpu_ik_paths_teacher_forced(arm_id, dtype, method):
    """65 rows, 60 steps, every stored step against one oracle step from the device's own position; float64 under the
    default limits: the free-running path within 1e-8 of oracle.ik_paths (the bound of test_rows_inverse_kinematics)"""
    for limits in ("default", "wide"):
        K.run_path(_run(arm_id, dtype), arm_id, dtype, method, 65, 60, K.SEED_PATH, limits, free_running=limits == "default")


# ---------------------------------------------------------------- (c) what holds on every row
@DTYPES
@pytest.mark.parametrize("arm_id", ("twojoint", "threejoint", "ur5", "synth7"))
def test_gpu_ik_properties_hold_on_singular_rows_along_a_path(arm_id, dtype):
    """8 steps from the 130-row draw, the 16 rows at multiples of pi / 2 among them: finite, within max_dq dt, the
    update a plain add in the dtype and the first position the input, bit for bit (tests/ik_cases.check_properties)"""
    q, tgt, block = K.draw_random(K.arm_table(arm_id), 130, K.SEED_STEP, dtype)
    assert (block == 0).sum() == K.N_SINGULAR
    for method in (1, 2, 3):
        for limits in ("default", "wide"):
            p = K.params(limits, method, T=8)
            pp, vp = _call(arm_id, p, q, tgt, dtype)
            K.check_properties(q, pp, vp, p, dtype)
            assert np.abs(vp[:K.N_SINGULAR]).max() > 0


# ---------------------------------------------------------------- (d) the Cholesky path of pinv_KxN and its fallback
@DTYPES
@pytest.mark.parametrize("arm_id,method", (("ur5", 1), ("ur5", 3), ("synth3", 3)))
def test_gpu_ik_fast_path_and_fallback_agree(arm_id, method, dtype):
    """pinv_KxN inverts through a K x K Cholesky factor where trace^K < det * 1e6 (float32: 1e2) and through the
    one-sided Jacobi SVD elsewhere, lane by lane.  Rows on both sides of that gate meet the same bar against the oracle;
    on rows that pass it with a factor 10 to spare (float32: 2 - trace^3 / det is 27 at the least, so 1e2 leaves no more),
    16 perturbations of q of one rounding each move the step by no more than the bar on top of what they move the
    oracle's.  Method 3 (3 x 3 blocks; synth3: K = N, and no exactly-zero Jacobian row as on the planar built-in, whose
    determinant is 0): both sides are populated.  Method 1:
    trace^6 / det >= 6^6 > 1e2 for every 6 x 6 matrix, so the float32 gate cannot pass, and it is above 9e6 at every one
    of 20 000 random UR5 postures, so the float64 one does not either: only the fallback side is populated."""
    dt = np.dtype(dtype)
    q, tgt, block, refs = K.one_step_case(arm_id, 130, K.SEED_STEP, dt.name, method)
    r, p = refs["wide"], K.params("wide", method)
    ok = K.counted(r, dt) & ((block != 0) if dt == K.F32 else True)
    fast = (r.gate < K.FAST_GATE[dt]).all(axis=1)
    pp, vp = _call(arm_id, p, q, tgt, dt)
    rat = K.ratio(r, vp[:, 0], dt)
    print(f"{arm_id} {dt.name} method {method}: {int((ok & fast).sum())} counted rows on the Cholesky path (worst error / bar "
          f"{rat[ok & fast].max(initial=0):.3g}), {int((ok & ~fast).sum())} on the fallback ({rat[ok & ~fast].max(initial=0):.3g})")
    assert (ok & ~fast).sum() > 0 and np.all(rat[ok] <= 1)
    if method == 1:
        assert not fast.any()
        return
    assert (ok & fast).sum() > 0
    room = ok & (r.gate < K.FAST_GATE[dt] / (10 if dt == K.F64 else 2)).all(axis=1)
    assert room.sum() > 0
    rng = np.random.RandomState(4)
    for k in range(16):
        qk = K._round(q * (1 + K.eps(dt) * rng.choice([-1.0, 1.0], q.shape)), dt)
        assert np.any(qk != q)
        rk = K.one_step(K.arm_table(arm_id), p, qk, tgt)
        _, vk = _call(arm_id, p, qk, tgt, dt)
        moved = np.abs(vk[:, 0].astype(float) - vp[:, 0].astype(float)).max(axis=1)
        allowed = K.bar(r, dt) + np.abs(rk.dq_ref - r.dq_ref).max(axis=1)
        use = room & K.counted(rk, dt)
        assert np.all(moved[use] <= allowed[use]), (k, (moved / allowed)[use].max())


@pytest.mark.parametrize("arm_id", ("synth3",))
def test_gpu_ik_next_to_a_singularity_float32(arm_id):
    """32 postures with kappa of 200 - 700, far beyond the float32 gate of the Cholesky path: held to the bar, which
    only the Jacobi fallback meets there (tests/ik_cases.run_ill)"""
    K.run_ill(_run(arm_id, np.float32), arm_id, np.float32, 32, 6)


# ---------------------------------------------------------------- (e) bits
@DTYPES
@pytest.mark.parametrize("arm_id", ("ur5", "threejoint", "ur5_rt"))
def test_gpu_ik_bits_do_not_depend_on_batch_placement_or_stream(arm_id, dtype):
    import abr_control_amd as a
    from abr_control_amd._lib import lib

    dt = np.dtype(dtype)
    be = _backend(arm_id)
    n, B, T = be.n, 130, 8
    q, tgt, _ = K.draw_random(K.arm_table(arm_id), B, K.SEED_STEP, dt)
    q, tgt = q.astype(dt), tgt.astype(dt)
    p = K.params("wide", 3, T=T)
    pp, vp = _call(arm_id, p, q, tgt, dt)
    assert pp.shape == (B, T, n) and np.abs(vp).max() > 0
    # rows of shorter batches: either side of a wavefront, and a single row
    for Bs in (1, 63, 64, 65):
        ps, vs = _call(arm_id, p, q[:Bs], tgt[:Bs], dt)
        assert np.array_equal(ps, pp[:Bs]) and np.array_equal(vs, vp[:Bs]), Bs
    # DeviceArrays; preallocated outputs on a stream of the caller's; outputs one row into a larger buffer
    s = a.Stream()
    qd, td = a.DeviceArray.from_numpy(q), a.DeviceArray.from_numpy(tgt)
    pd, vd = _call(arm_id, p, qd, td, dt)
    assert np.array_equal(pd.numpy(), pp) and np.array_equal(vd.numpy(), vp)
    nan = np.full((B + 1, T, n), np.nan, dt)
    big_p, big_v = a.DeviceArray.from_numpy(nan), a.DeviceArray.from_numpy(nan)
    pre_p, pre_v = a.DeviceArray.from_numpy(nan[1:]), a.DeviceArray.from_numpy(nan[1:])
    _call(arm_id, p, qd, td, dt, stream=s, position_path=pre_p, velocity_path=pre_v)
    _call(arm_id, p, qd, td, dt, stream=s, position_path=big_p.rows(1, B + 1), velocity_path=big_v.rows(1, B + 1))
    s.sync()
    assert np.array_equal(pre_p.numpy(), pp) and np.array_equal(pre_v.numpy(), vp)
    for big, ref in ((big_p, pp), (big_v, vp)):
        h = big.numpy()
        assert np.array_equal(h[1:], ref) and np.all(np.isnan(h[0]))
    # the compiled plugin of the same table runs the built-in's kernels
    if arm_id == "ur5":
        pc, vc = _call("ur5_compiled", p, q, tgt, dt)
        assert np.array_equal(pc, pp) and np.array_equal(vc, vp)
    # no steps: nothing is written (the C entry itself; the Python layer would size the outputs [B, 0, n])
    p0 = K.params("wide", 3, T=0)
    hp, hv = nan[1:].copy(), nan[1:].copy()
    rc = lib().abrk_ik_generate_path_batch(be.arm_id, _abi.F64 if dt == K.F64 else _abi.F32, C.byref(p0), B, q.ctypes.data,
                                           tgt.ctypes.data, hp.ctypes.data, hv.ctypes.data, 0, None)
    assert rc == 0 and np.all(np.isnan(hp)) and np.all(np.isnan(hv))
    rc = lib().abrk_ik_generate_path_batch(be.arm_id, _abi.F64 if dt == K.F64 else _abi.F32, C.byref(p0), B, qd.ptr, td.ptr,
                                           pre_p.ptr, pre_v.ptr, 0, s.ptr)
    s.sync()
    assert rc == 0 and np.array_equal(pre_p.numpy(), pp) and np.array_equal(pre_v.numpy(), vp)


@DTYPES
@pytest.mark.parametrize("arm_id", ("threejoint", "synth7"))
def test_gpu_ik_outputs_at_unaligned_addresses(arm_id, dtype):
    """T = 7 with 3 and with 7 joints: a row of a path is 7 n elements, so outputs that begin one row into a buffer sit
    at an address that is no multiple of 16 bytes (nor, in float32 with 7 joints, of 8)"""
    import abr_control_amd as a

    dt = np.dtype(dtype)
    n, B, T = _backend(arm_id).n, 65, 7
    assert (T * n * dt.itemsize) % 16 != 0
    q, tgt, _ = K.draw_random(K.arm_table(arm_id), B, K.SEED_STEP, dt)
    q, tgt = q.astype(dt), tgt.astype(dt)
    p = K.params("wide", 3, T=T)
    pp, vp = _call(arm_id, p, q, tgt, dt)
    nan = np.full((B + 2, T, n), np.nan, dt)
    big_p, big_v = a.DeviceArray.from_numpy(nan), a.DeviceArray.from_numpy(nan)
    _call(arm_id, p, a.DeviceArray.from_numpy(q), a.DeviceArray.from_numpy(tgt), dt, position_path=big_p.rows(1, B + 1),
          velocity_path=big_v.rows(1, B + 1))
    for big, ref in ((big_p, pp), (big_v, vp)):
        h = big.numpy()
        assert np.array_equal(h[1:-1], ref) and np.all(np.isnan(h[0])) and np.all(np.isnan(h[-1]))


# ---------------------------------------------------------------- (f) convergence
def _numpy_float32_end(tab, p, q0, tgt):
    """the free-running iteration with the reference's formulas in NumPy float32 (J, Tx and the quaternion from the
    oracle at the float32 position, rounded to float32; K.numpy_step; q += dq in float32) -> the last stored position"""
    q = q0.astype(np.float32)
    for _ in range(int(p.n_timesteps) - 1):
        r = K.one_step(tab, p, q.astype(np.float64), tgt)
        dq, _, _ = K.numpy_step(K._round(r.J, K.F32), K._round(r.dx, K.F32), K._round(r.dr, K.F32), 3, r.lim["dq"], K.F32)
        q = q + dq
    return q.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _convergence_case(arm_id):
    from oracle import oracle as O

    tab = K.arm_table(arm_id)
    q0, tgt = K.draw_reachable(tab, 64, 21, K.F32)  # float32-representable: both dtypes run the same inputs
    p = K.params("default", 3, T=200, max_dx=5.0, max_dq=4 * np.pi)
    o = O.Oracle(tab)
    end_error = lambda qe: np.linalg.norm(K._tx(o, qe) - tgt[:, :3], axis=1)
    e0, e_or = end_error(q0), end_error(O.ik_paths(tab, p, q0, tgt)[0][:, -1])
    e_np = end_error(_numpy_float32_end(tab, p, q0, tgt))
    return q0, tgt, p, end_error, e0, e_or, float(np.abs(e_np - e_or).max())


@DTYPES
@pytest.mark.parametrize("arm_id", ("ur5", "jaco2"))
def test_gpu_ik_converges_on_reachable_targets(arm_id, dtype):
    """what the class is for: from 1 - 40 cm away, 200 steps of method 3 (max_dx = 5, max_dq = 4 pi) end where the
    oracle's do.  float64: within 1e-9 m of the oracle's end error, per row; float32: within four times the difference
    the reference's formulas in NumPy float32 show end to end on the same rows"""
    dt = np.dtype(dtype)
    q0, tgt, p, end_error, e0, e_or, d_np = _convergence_case(arm_id)
    assert e0.min() > 0.01 and np.median(e_or) < 1e-5 and e_or.max() < 1e-4
    pp, vp = _call(arm_id, p, q0.astype(dt), tgt.astype(dt), dt)
    e = end_error(pp[:, -1].astype(np.float64))
    slack = 1e-9 if dt == K.F64 else 4 * d_np
    print(f"{arm_id} {dt.name}: start {e0.min():.2f} - {e0.max():.2f} m; oracle ends at median {np.median(e_or):.2e} worst "
          f"{e_or.max():.2e}; device median {np.median(e):.2e} worst {e.max():.2e}; worst excess {np.max(e - e_or):.2e} "
          f"(allowed {slack:.2e}; NumPy float32 differs by {d_np:.2e})")
    assert np.all(e <= e_or + slack)


# ---------------------------------------------------------------- (g) the class
def test_gpu_ik_class_with_two_and_seven_joints():
    from abr_control_amd import arms, engine
    from abr_control_amd.controllers.path_planners import InverseKinematics

    for rc, tab in ((arms.twojoint.Config(), _abi.load_table("twojoint")), (arms.from_table(K.synthetic(7)), K.synthetic(7))):
        n, B, T = rc.N_JOINTS, 5, 12
        q0, tgt = K.draw_reachable(tab, B, 9, np.float64)
        ik = InverseKinematics(rc, max_dx=50.0, max_dr=300.0, max_dq=2000.0)
        pp, vp = ik.generate_path(q0, tgt, n_timesteps=T, method=3)
        assert pp.shape == (B, T, n) and vp.shape == (B, T, n)
        ref = engine.ik_generate_path(rc.arm_id, n, K.params("wide", 3, T=T), q0, tgt, device=rc.device)
        assert np.array_equal(pp, ref[0]) and np.array_equal(vp, ref[1]) and np.abs(vp).max() > 0
        for t in list(range(T)) + [T - 1, T - 1]:  # next() walks the path and stays on its last step
            pos, vel = ik.next()
            assert np.array_equal(pos, pp[:, t]) and np.array_equal(vel, vp[:, t])
        p1, v1 = ik.generate_path(q0[3], tgt[3], n_timesteps=T, method=3)  # one path: the reference's shapes
        assert p1.shape == (T, n) and np.array_equal(p1, pp[3]) and np.array_equal(v1, vp[3])
        pos, vel = ik.next()
        assert pos.shape == (n,) and np.array_equal(pos, p1[0]) and ik.n == 1
