"""Parity tests proper: libabrk.so (HIP kernels on the MI355X) through the C ABI against
(a) the reference-generated golden vectors, (b) the CPU oracle on fresh seeded inputs,
(c) size-independent properties at BASELINE.json's full batch sizes.  `-m gpu` only."""
import os

import numpy as np
import pytest

from abr_control_amd import _abi
from tests import cases
from tests.conftest import golden

pytestmark = pytest.mark.gpu

ARMS = ["twojoint", "threejoint", "ur5", "jaco2"]
DYN_ARMS = ARMS + ["onejoint"]  # N_LINKS = 1: kinematics of every frame, M = g = C = 0


def draw(seed, B, n, nt=6):
    """the reference benchmark's input distribution (examples/timing_plots.py:18-20)"""
    rng = np.random.RandomState(seed)
    return rng.uniform(0, 2 * np.pi, (B, n)), rng.uniform(0, 5, (B, n)), rng.uniform(-1, 1, (B, nt))


def test_native_library_is_loaded():
    import abr_control_amd as a

    assert a.device_count() >= 1
    assert "gfx950" in a.device_name(0)
    maps = open("/proc/self/maps").read()
    assert "libabrk.so" in maps, "the HIP extension is not the one running"


@pytest.mark.parametrize("variant", ["static", "rt"])
@pytest.mark.parametrize("arm", DYN_ARMS)
def test_gpu_dynamics_match_reference(arm, variant):
    cases.check_dynamics_against_golden(cases.GpuBackend(arm, variant), arm, golden(arm))


@pytest.mark.parametrize("case_id", sorted(cases.CASES))
def test_gpu_controllers_match_reference(case_id):
    arm = cases.CASES[case_id]["arm"]
    cases.check_case_against_golden(cases.GpuBackend(arm, "static"), case_id, golden(arm))


@pytest.mark.parametrize("case_id", ["twojoint:cfg1", "ur5:cfg2", "ur5:cfg4", "ur5:osc6_alg0", "ur5:osc_null2",
                                     "ur5:sliding", "jaco2:cfg3", "jaco2:osc6_alg1", "threejoint:cfg5", "ur5:joint"])
def test_gpu_runtime_table_arms(case_id):
    arm = cases.CASES[case_id]["arm"]
    cases.check_case_against_golden(cases.GpuBackend(arm, "rt"), case_id, golden(arm))


def test_gpu_fp32_config5_full_size():
    """BASELINE config 5: threejoint Sliding, batch 65536, fp32, tolerance 1e-4"""
    g = golden("threejoint")
    be = cases.GpuBackend("threejoint")
    # golden sample (reference as shipped)
    u, _ = cases.run_case(be, cases.CASES["threejoint:cfg5"], g, dtype=np.float32)
    q = g["cfg5_q"]
    well = (np.abs(np.sin(q[:, 1])) > 0.05) & (np.abs(np.sin(q[:, 2])) > 0.05)
    assert cases.rel_err(u.astype(float), g["cfg5_uS"])[well].max() <= cases.TOL_F32
    # full size vs the fp64 kernel (itself pinned above) + oracle on a sample
    B = 65536
    q, dq, t = draw(5, B, 3, 3)
    p = _abi.make_sliding_params(3)
    u32, _ = be.sliding(p, q, dq, t, dtype=np.float32)
    u64, _ = be.sliding(p, q, dq, t)
    well = (np.abs(np.sin(q[:, 1])) > 0.05) & (np.abs(np.sin(q[:, 2])) > 0.05)
    assert np.all(np.isfinite(u32))
    assert cases.rel_err(u32.astype(float), u64)[well].max() <= cases.TOL_F32
    uo, _ = cases.OracleBackend("threejoint").sliding(p, q[:4096], dq[:4096], t[:4096])
    assert cases.rel_err(u64[:4096], uo).max() <= 1e-6


# float32 is the reference's own shipped precision for J, M, g, C, dJ, R (base_config.py:223,247,270,285,301,336): every
# `float` instantiation a user reaches through Config(dtype=np.float32) meets the reference's outputs on the device
FP32_CASES = ["twojoint:cfg1", "ur5:cfg2", "ur5:cfg4", "jaco2:cfg3", "ur5:osc6_alg0", "jaco2:osc6_alg1", "ur5:osc_null2",
              "ur5:osc_xyz_tvel", "ur5:joint", "jaco2:damping", "ur5:sliding", "threejoint:cfg5"]


@pytest.mark.parametrize("variant", ["static", "rt"])
@pytest.mark.parametrize("case_id", FP32_CASES)
def test_gpu_fp32_kernels_match_reference(case_id, variant):
    """the fp32 OSC / Joint / Sliding kernels against the reference's fp64 formulas at TOL_F32 = 1e-4 on the rows whose
    Mx_inv is well conditioned (cases.check_case_against_golden: cond < 1e3, six task rows < 1e4 + a cond-scaled bound)"""
    arm = cases.CASES[case_id]["arm"]
    r = cases.check_case_against_golden(cases.GpuBackend(arm, variant), case_id, golden(arm), dtype=np.float32)
    assert r["worst_vs_D"] <= cases.TOL_F32


@pytest.mark.parametrize("variant", ["static", "rt"])
@pytest.mark.parametrize("arm", DYN_ARMS)
def test_gpu_fp32_dynamics_match_reference(arm, variant):
    """every robot_config function of every frame in fp32 (2e-4 of the array's scale)"""
    cases.check_dynamics_against_golden(cases.GpuBackend(arm, variant), arm, golden(arm), dtype=np.float32)


def test_gpu_fp32_config2_full_size_vs_fp64_kernel():
    """2^20 rows of BASELINE config 2's law: the float kernel against the double kernel (itself pinned to the reference)
    on the rows whose 3 x 3 Mx_inv is well conditioned, and bounded by its conditioning on all others"""
    be = cases.GpuBackend("ur5")
    p = _abi.make_osc_params(6, kp=200)
    B = 1 << 20
    q, dq, t = draw(7, B, 6)
    q32, dq32, t32 = (a.astype(np.float32) for a in (q, dq, t))
    u32, _ = be.osc(p, q32, dq32, t32, dtype=np.float32)
    # the same float32-representable states through the double kernel: what is compared is the arithmetic
    u64, _ = be.osc(p, q32.astype(float), dq32.astype(float), t32.astype(float))
    assert u32.dtype == np.float32 and np.all(np.isfinite(u32))
    r = be.dynamics(q32.astype(float), None, "EE", None, ("J", "M"))
    A = np.einsum("bij,bjk,blk->bil", r["J"][:, :3], np.linalg.inv(r["M"]), r["J"][:, :3])
    sv = np.linalg.eigvalsh(A)
    cond = sv[:, -1] / np.maximum(sv[:, 0], 1e-300)
    det = np.abs(np.linalg.det(A))
    err = cases.rel_err(u32.astype(float), u64)
    well = cond < 1e3
    assert well.mean() > 0.4
    assert err[well].max() <= cases.TOL_F32, err[well].max()
    # away from the two thresholds of _Mx (osc.py:138,145: the float kernel may take the other branch next to them)
    clear = (np.abs(det - 1e-3) > 1e-4) & (np.abs(sv[:, 0] / sv[:, -1] - 1e-4) > 3e-5) & (cond < 1e6)
    assert (err[clear] <= np.maximum(cases.TOL_F32, 1e-6 * cond[clear])).all(), \
        (err[clear] / np.maximum(cases.TOL_F32, 1e-6 * cond[clear])).max()


def test_gpu_config2_config4_full_size_vs_oracle():
    """BASELINE configs 2 (B=4096) and 4 (B=2^20 on one GPU): oracle on a sample + properties"""
    be, orc = cases.GpuBackend("ur5"), cases.OracleBackend("ur5")
    p2 = _abi.make_osc_params(6, kp=200)
    p4 = _abi.make_osc_params(6, kp=200, use_g=True, use_C=True)
    q, dq, t = draw(1, 4096, 6)
    u, _ = be.osc(p2, q, dq, t)
    uo, _ = orc.osc(p2, q, dq, t)
    assert cases.rel_err(u, uo).max() <= 1e-6
    B = 1 << 20
    q, dq, t = draw(2, B, 6)
    u, ts = be.osc(p4, q, dq, t)
    assert np.all(np.isfinite(u))
    idx = np.random.RandomState(0).choice(B, 4096, replace=False)
    uo, _ = orc.osc(p4, q[idx], dq[idx], t[idx])
    assert cases.rel_err(u[idx], uo).max() <= 1e-6
    # rows are independent: any sub-batch / permutation reproduces the same bits
    perm = np.random.RandomState(1).permutation(B)[:100003]
    u_sub, _ = be.osc(p4, q[perm], dq[perm], t[perm])
    assert np.array_equal(u_sub, u[perm])
    # u = training_signal - g   (osc.py:297-301)
    gq = be.dynamics(q[:65536], None, "EE", None, ("g",))["g"]
    assert np.allclose(u[:65536], ts[:65536] - gq, rtol=1e-12, atol=1e-12)
    # use_C only subtracts C(q,dq) dq (osc.py:291-292)
    u_noC, _ = be.osc(_abi.make_osc_params(6, kp=200), q[:65536], dq[:65536], t[:65536])
    Cq = be.dynamics(q[:65536], dq[:65536], "EE", None, ("C",))["C"]
    assert np.allclose(u_noC - np.einsum("bij,bj->bi", Cq, dq[:65536]), u[:65536], rtol=1e-10, atol=1e-9)


def test_gpu_config3_full_size():
    """BASELINE config 3: Jaco2 OSC + null-space Damping, batch 16384"""
    be, orc = cases.GpuBackend("jaco2"), cases.OracleBackend("jaco2")
    p = _abi.make_osc_params(6, kp=200, null_controllers=[_abi.make_damping(10)])
    q, dq, t = draw(0, 16384, 6)
    u, _ = be.osc(p, q, dq, t)
    uo, _ = orc.osc(p, q[:2048], dq[:2048], t[:2048])
    assert cases.rel_err(u[:2048], uo).max() <= 1e-6
    # the filtered damping term does not accelerate the task point: J M^-1 (u_damped - u_plain) = 0
    # wherever Mx is the true inverse of Mx_inv (i.e. not the truncated pinv of osc.py:145)
    u0, _ = be.osc(_abi.make_osc_params(6, kp=200), q, dq, t)
    r = be.dynamics(q, None, "EE", None, ("J", "M"))
    J3, du = r["J"][:, :3], u - u0
    Minv_du = np.linalg.solve(r["M"], du[..., None])[..., 0]
    acc = np.einsum("bij,bj->bi", J3, Minv_du)
    A = np.einsum("bij,bjk,blk->bil", J3, np.linalg.inv(r["M"]), J3)
    ok = (np.linalg.cond(A) < 1e3) & (np.linalg.cond(r["M"]) < 1e6)
    ref = np.abs(np.einsum("bij,bj->bi", J3, np.linalg.solve(r["M"], (u0 - u)[..., None])[..., 0])).max()
    assert ok.mean() > 0.5
    assert np.abs(acc[ok]).max() < 1e-9 * max(1.0, np.abs(Minv_du).max())


def test_gpu_dynamics_properties_large_batch():
    be = cases.GpuBackend("ur5")
    B = 200_000
    q, dq, _ = draw(3, B, 6)
    r = be.dynamics(q, dq, "EE", None, ("M", "C", "J", "dJ", "g", "R", "quat", "T", "Tinv"))
    M = r["M"]
    assert np.array_equal(M, M.transpose(0, 2, 1))                       # exactly symmetric
    assert np.linalg.eigvalsh(M[:20000]).min() > 0                         # positive definite
    # Mdot - 2C skew-symmetric (Christoffel form), checked with a central difference of M
    h = 1e-6
    Mp = be.dynamics(q[:4096] + h * dq[:4096], None, "EE", None, ("M",))["M"]
    Mm = be.dynamics(q[:4096] - h * dq[:4096], None, "EE", None, ("M",))["M"]
    N = (Mp - Mm) / (2 * h) - 2 * r["C"][:4096]
    assert np.abs(N + N.transpose(0, 2, 1)).max() < 1e-5
    # dJ is the directional derivative of J
    Jp = be.dynamics(q[:4096] + h * dq[:4096], None, "EE", None, ("J",))["J"]
    Jm = be.dynamics(q[:4096] - h * dq[:4096], None, "EE", None, ("J",))["J"]
    assert np.abs((Jp - Jm) / (2 * h) - r["dJ"][:4096]).max() < 1e-5
    # rotations orthonormal, quaternion consistent with R, T_inv T = I
    R = r["R"]
    assert np.abs(np.einsum("bij,bkj->bik", R, R) - np.eye(3)).max() < 1e-13
    w, x, y, z = r["quat"].T
    assert np.allclose(w * w + x * x + y * y + z * z, 1.0, atol=1e-14) and (w >= 0).all()
    assert np.allclose(1 - 2 * (y * y + z * z), R[:, 0, 0], atol=1e-12)
    assert np.abs(np.einsum("bij,bjk->bik", r["Tinv"], r["T"]) - np.eye(4)).max() < 1e-13


def test_gpu_batch_edges_and_device_arrays():
    import abr_control_amd as a
    from abr_control_amd import engine

    be, orc = cases.GpuBackend("ur5"), cases.OracleBackend("ur5")
    p = _abi.make_osc_params(6, kp=200)
    for B in (1, 63, 64, 65, 1000):
        q, dq, t = draw(B, B, 6)
        u, _ = be.osc(p, q, dq, t)
        uo, _ = orc.osc(p, q, dq, t)
        assert u.shape == (B, 6) and cases.rel_err(u, uo).max() <= 1e-6
    # empty batch
    assert be.osc(p, np.zeros((0, 6)), np.zeros((0, 6)), np.zeros((0, 6)))[0].shape == (0, 6)
    # device-resident arrays: zero-copy, same bits as the staged host path
    q, dq, t = draw(9, 5000, 6)
    dq_, q_, t_ = a.DeviceArray.from_numpy(dq), a.DeviceArray.from_numpy(q), a.DeviceArray.from_numpy(t)
    ud = engine.osc_generate(be.arm_id, 6, p, q_, dq_, t_)
    assert isinstance(ud, a.DeviceArray)
    assert np.array_equal(ud.numpy(), be.osc(p, q, dq, t)[0])
    # explicit stream
    s = a.Stream(0)
    ud2 = engine.osc_generate(be.arm_id, 6, p, q_, dq_, t_, stream=s)
    s.sync()
    assert np.array_equal(ud2.numpy(), ud.numpy())
    with pytest.raises(TypeError):
        engine.osc_generate(be.arm_id, 6, p, q_, dq, t)


def test_gpu_singular_inertia_matrix_is_reported():
    """a joint-space inertia matrix that is not positive definite (a user arm whose last link has neither mass nor
    inertia: M's last row and column are zero) - the reference's np.linalg.inv(M) raises LinAlgError (osc.py:136); here a
    host-array call returns ABRK_ESINGULAR (a LinAlgError in Python), a device-pointer call leaves the flag for the next
    abrk_stream_sync of its device, which reports it once.  Non-finite states are NOT singular (inv returns NaNs), and
    nothing sticks to later calls."""
    import abr_control_amd as a
    from abr_control_amd import engine
    from abr_control_amd._lib import SingularMatrixError
    from tests.synthetic_arms import make_arm

    tab = make_arm(6, 77)
    tab["mdiag"][6] = [0.0] * 6  # the last link: no mass, no inertia
    bad = cases.GpuBackend(tab)
    good = cases.GpuBackend(make_arm(6, 77))
    q, dq, t = draw(5, 300, 6)
    laws = (_abi.make_osc_params(6, kp=100), _abi.make_osc_params(6, kp=100, use_C=True),
            _abi.make_osc_params(6, kp=100, ko=80, ctrlr_dof=[1] * 6),
            _abi.make_osc_params(6, kp=100, null_controllers=[_abi.make_damping(5)]))
    for p in laws:
        for dtype in (np.float64, np.float32):
            with pytest.raises(np.linalg.LinAlgError) as ei:
                bad.osc(p, q, dq, t, dtype=dtype)
            assert isinstance(ei.value, SingularMatrixError) and ei.value.code == _abi.ESINGULAR
            assert "Singular matrix" in str(ei.value)
            u, _ = good.osc(p, q, dq, t, dtype=dtype)  # the same thread's next call: nothing sticks
            assert np.isfinite(u).all()
    # non-finite inputs give non-finite outputs, not an error (numpy.linalg.inv does not raise on NaN either)
    qn = q.copy()
    qn[7, 1] = np.nan
    u, _ = good.osc(laws[0], qn, dq, t)
    assert np.isnan(u[7]).any() and np.isfinite(np.delete(u, 7, axis=0)).all()
    # device pointers: the call is asynchronous, the flag is the device's and abrk_stream_sync reports it - once
    s = a.Stream(0)
    q_, dq_, t_ = (a.DeviceArray.from_numpy(x) for x in (q, dq, t))
    engine.osc_generate(bad.arm_id, 6, laws[0], q_, dq_, t_, stream=s)
    with pytest.raises(np.linalg.LinAlgError):
        s.sync()
    s.sync()
    ud = engine.osc_generate(good.arm_id, 6, laws[0], q_, dq_, t_, stream=s)
    s.sync()
    assert np.array_equal(ud.numpy(), good.osc(laws[0], q, dq, t)[0])
    # host batches over shards (abrk_osc_generate_sharded): the call reports its own batch, x,y,z and six-row law alike
    from abr_control_amd.sharding import MultiDevice

    devices = [0, 0, 0]
    for p in (laws[0], laws[2]):
        with pytest.raises(np.linalg.LinAlgError) as ei:
            engine.osc_generate_sharded(bad.arm_id, 6, p, q, dq, t, devices)
        assert isinstance(ei.value, SingularMatrixError) and ei.value.code == _abi.ESINGULAR
        us = engine.osc_generate_sharded(good.arm_id, 6, p, q, dq, t, devices)  # nothing sticks
        assert np.array_equal(us, engine.osc_generate(good.arm_id, 6, p, q, dq, t))
    # ... and nothing a resident call left on the library's shard streams (the same streams): that flag stays for the
    # resident batch's own sync, which reports it once
    md = MultiDevice(devices)
    qs, dqs, ts_ = (md.scatter(x) for x in (q, dq, t))
    engine.osc_generate_resident(bad.arm_id, 6, laws[0], qs, dqs, ts_)
    engine.osc_generate_sharded(good.arm_id, 6, laws[0], q, dq, t, devices)
    with pytest.raises(np.linalg.LinAlgError):
        md.sync()
    md.sync()


def test_gpu_singular_flag_is_per_stream():
    """ADVICE r5 / VERDICT r5 weak #3: several control loops on one GPU.  A singular batch enqueued on stream A is reported
    by what drains stream A - Stream.sync, DeviceArray.numpy(stream A), abrk_device_sync - and never by another stream's
    sync, whichever comes first, from whichever thread; the healthy loop's results are untouched."""
    import threading

    import abr_control_amd as a
    from abr_control_amd import engine
    from abr_control_amd._lib import check, lib
    from tests.synthetic_arms import make_arm

    tab = make_arm(6, 77)
    tab["mdiag"][6] = [0.0] * 6
    bad, good = cases.GpuBackend(tab), cases.GpuBackend(make_arm(6, 77))
    q, dq, t = draw(5, 300, 6)
    p = _abi.make_osc_params(6, kp=100)
    p6 = _abi.make_osc_params(6, kp=100, ko=80, ctrlr_dof=[1] * 6)
    want = good.osc(p, q, dq, t)[0]
    sa, sb = a.Stream(0), a.Stream(0)
    q_, dq_, t_ = (a.DeviceArray.from_numpy(x) for x in (q, dq, t))
    for law in (p, p6):
        ua = engine.osc_generate(bad.arm_id, 6, law, q_, dq_, t_, stream=sa)
        ub = engine.osc_generate(good.arm_id, 6, p, q_, dq_, t_, stream=sb)
        sb.sync()                              # the healthy loop syncs FIRST: it must not be handed A's flag
        assert np.array_equal(ub.numpy(sb), want)
        with pytest.raises(np.linalg.LinAlgError):
            sa.sync()
        sa.sync()                              # reported once
    # read-back instead of a sync: the copy drains the stream and reports
    ua = engine.osc_generate(bad.arm_id, 6, p, q_, dq_, t_, stream=sa)
    with pytest.raises(np.linalg.LinAlgError):
        ua.numpy(sa)
    sa.sync()
    # abrk_device_sync: any stream of the device
    engine.osc_generate(bad.arm_id, 6, p, q_, dq_, t_, stream=sa)
    with pytest.raises(np.linalg.LinAlgError):
        check(lib().abrk_device_sync(0))
    sa.sync()
    sb.sync()
    # two threads, one loop each, many ticks: only the singular loop's thread ever sees the error
    seen = {"bad": 0, "good": 0, "good_results_ok": True}

    def loop(which, arm_id, stream):
        for _ in range(40):
            u = engine.osc_generate(arm_id, 6, p, q_, dq_, t_, stream=stream)
            try:
                stream.sync()
                if which == "good" and not np.array_equal(u.numpy(stream), want):
                    seen["good_results_ok"] = False
            except np.linalg.LinAlgError:
                seen[which] += 1

    ths = [threading.Thread(target=loop, args=("bad", bad.arm_id, sa)), threading.Thread(target=loop, args=("good", good.arm_id, sb))]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert seen == {"bad": 40, "good": 0, "good_results_ok": True}, seen
    # a destroyed stream hands its word back; a new stream starts clean even if the handle value is reused
    engine.osc_generate(bad.arm_id, 6, p, q_, dq_, t_, stream=sa)
    del sa
    sc = a.Stream(0)
    engine.osc_generate(good.arm_id, 6, p, q_, dq_, t_, stream=sc)
    sc.sync()
    # host-array calls from short-lived threads: each thread's pinned word returns to the pool when the thread exits
    def host_call():
        good.osc(p, q[:8], dq[:8], t[:8])

    before = _abi.ScratchInfo()
    check(lib().abrk_scratch_stats(0, before))
    for _ in range(200):
        th = threading.Thread(target=host_call)
        th.start()
        th.join()
    info = _abi.ScratchInfo()
    check(lib().abrk_scratch_stats(0, info))
    # (relative to what the process held before: other tests' live streams and threads keep their words)
    assert info.status_words_out <= before.status_words_out + 1, (before.status_words_out, info.status_words_out)
    assert info.status_blocks <= before.status_blocks + 1, (before.status_blocks, info.status_blocks)


def test_gpu_python_api_drop_in():
    """robot_config / controller classes: reference shapes, dtypes and per-call state"""
    from abr_control_amd.arms import jaco2, threejoint, twojoint, ur5
    from abr_control_amd.controllers import OSC, Damping, Joint, RestingConfig, Sliding

    g = golden("ur5")
    rc = ur5.Config(use_cython=True)
    q, dq = g["dyn_q"], g["dyn_dq"]
    # single state: reference dtypes (float32 casts at base_config.py:223-336; Tx float64)
    J = rc.J("EE", q[5])
    assert J.shape == (6, 6) and J.dtype == np.float32
    assert np.allclose(J, g["J_EE"][5].astype(np.float32), rtol=2e-7, atol=1e-7)
    M = rc.M(q[5])
    assert M.dtype == np.float32 and np.allclose(M, g["M"][5].astype(np.float32), rtol=2e-7)
    assert rc.g(q[5]).dtype == np.float32 and rc.g(q[5]).shape == (6,)
    assert rc.C(q[5], dq[5]).shape == (6, 6) and rc.dJ("EE", q[5], dq[5]).shape == (6, 6)
    Tx = rc.Tx("EE", q[5])
    assert Tx.dtype == np.float64 and Tx.shape == (3,) and np.allclose(Tx, g["Tx_EE"][5], atol=1e-14)
    assert np.allclose(rc.Tx("EE", q[5], x=g["xoff"]), g["Tx_EE_x"][5], atol=1e-14)
    assert rc.R("EE", q[5]).shape == (3, 3) and rc.T("EE", q[5]).shape == (4, 4)
    assert np.allclose(rc.quaternion("EE", q[5]), g["quat_EE"][5], atol=1e-12)
    assert np.allclose(rc.Tx("link3", q[5]), g["Tx_link3"][5], atol=1e-14)
    with pytest.raises(Exception, match="Invalid transformation name"):
        rc.Tx("link9", q[5])
    # batch
    assert rc.M(q).shape == (len(q), 6, 6) and rc.Tx("EE", q).shape == (len(q), 3)
    d = rc.dynamics(q, dq, want=("Tx", "J", "M", "g", "C"))
    assert np.allclose(d["C"], g["C"], atol=1e-12)

    # OSC single-call == golden (Oracle-D) and state handling of ki (osc.py:81-82, 262-264)
    c = OSC(rc, kp=200)
    u = c.generate(g["cfg2_q"][0], g["cfg2_dq"][0], g["cfg2_target"][0])
    assert u.shape == (6,) and u.dtype == np.float64
    assert cases.rel_err(u[None], g["cfg2_uD"][:1]).max() < 1e-6
    assert np.allclose(c.training_signal, g["cfg2_tsD"][0], rtol=1e-9)
    ub = c.generate(g["cfg2_q"], g["cfg2_dq"], g["cfg2_target"])
    assert cases.rel_err(ub, g["cfg2_uD"]).max() < 1e-6
    key = "osc_xyz_vmax_ki"
    c = OSC(rc, kp=100, kv=15, ki=0.2, ctrlr_dof=[True] * 3 + [False] * 3, vmax=[0.5, 1.0])
    for s in range(5):
        u = c.generate(g[f"{key}_q"][3], g[f"{key}_dq"][3], g[f"{key}_target"][3])
        assert cases.rel_err(u[None], g[f"{key}_uD"][s, 3][None]).max() < 1e-6
    assert c.integrated_error.shape == (6,)
    # fused + Python null controllers (osc.py:310-318)
    class PyDamping:
        def __init__(self, rc_, kv):
            self.rc, self.kv = rc_, kv

        def generate(self, q_, dq_):
            return np.dot(self.rc.M(q_).astype(float), -self.kv * dq_)

    key = "osc_null2"
    rest = RestingConfig(rc, [None, 0.8, -1.6, None, 1.5, None], kp=40, kv=8)
    c = OSC(rc, kp=200, null_controllers=[Damping(rc, 10), rest])
    u = c.generate(g[f"{key}_q"], g[f"{key}_dq"], g[f"{key}_target"])
    assert cases.rel_err(u, g[f"{key}_uD"]).max() < 1e-6
    c = OSC(rc, kp=200, null_controllers=[PyDamping(rc, 10), rest])
    u = c.generate(g[f"{key}_q"][:16], g[f"{key}_dq"][:16], g[f"{key}_target"][:16])
    assert cases.rel_err(u, g[f"{key}_uS"][:16]).max() < 1e-4  # float32 M in the Python controller
    # other controllers
    assert cases.rel_err(Joint(rc, kp=50, kv=9).generate(g["joint_q"], g["joint_dq"], g["joint_target"] * 3.0),
                         g["joint_uD"]).max() < 1e-6
    sl = Sliding(rc)
    u = sl.generate(g["sliding_q"][0], g["sliding_dq"][0], g["sliding_target"][0])
    assert u.shape == (6,) and sl.s.shape == (6,)
    assert cases.rel_err(u[None], g["sliding_uD"][:1]).max() < 1e-6
    g2 = golden("jaco2")
    rj = jaco2.Config()
    assert cases.rel_err(Damping(rj, 10).generate(g2["damping_q"], g2["damping_dq"]), g2["damping_uD"]).max() < 1e-6
    # twojoint config 1: batch of one through the public classes
    g1 = golden("twojoint")
    c1 = OSC(twojoint.Config(), kp=10, kv=3, ctrlr_dof=[True, True, False, False, False, False])
    u = c1.generate(g1["cfg1_q"][0], g1["cfg1_dq"][0], g1["cfg1_target"][0])
    assert cases.rel_err(u[None], g1["cfg1_uD"][:1]).max() < 1e-6
    # fp32 config
    g3 = golden("threejoint")
    s32 = Sliding(threejoint.Config(dtype=np.float32, reference_dtypes=False))
    u = s32.generate(g3["cfg5_q"][:64], g3["cfg5_dq"][:64], g3["cfg5_target"][:64])
    assert u.dtype == np.float32


def test_gpu_user_arm_from_table_matches_builtin():
    from abr_control_amd import arms
    from abr_control_amd.controllers import OSC

    tab = _abi.load_table("jaco2")
    user = arms.from_table(tab)
    builtin = arms.jaco2.Config()
    q, dq, t = draw(11, 3000, 6)
    a = OSC(user, kp=200).generate(q, dq, t)
    b = OSC(builtin, kp=200).generate(q, dq, t)
    assert cases.rel_err(a, b).max() < 1e-9


def test_gpu_nonfinite_and_huge_inputs():
    """NaN / Inf states must not turn into finite torques (the kernels are built with
    -ffinite-math-only for constant folding: documented behaviour, pinned here); angles beyond
    1e5 rad take the library sincos path and still match the oracle."""
    be, orc = cases.GpuBackend("ur5"), cases.OracleBackend("ur5")
    q, dq, t = draw(21, 256, 6)
    qn = q.copy()
    qn[3, 2] = np.nan
    qn[10, 0] = np.inf
    dqn = dq.copy()
    dqn[20, 5] = np.nan
    tn = t.copy()
    tn[30, 1] = np.nan
    for p in (_abi.make_osc_params(6, kp=200), _abi.make_osc_params(6, kp=200, use_C=True),
              _abi.make_osc_params(6, kp=50, ctrlr_dof=[1] * 6)):
        u, _ = be.osc(p, qn, dqn, tn)
        bad = [3, 10, 20, 30]
        assert np.isnan(u[bad]).any(axis=1).all(), "a non-finite state produced a finite control signal"
        good = np.setdiff1d(np.arange(256), bad)
        uo, _ = orc.osc(p, q[good], dq[good], t[good])
        assert cases.rel_err(u[good], uo).max() <= 1e-6  # neighbours in the same wavefront are unaffected
    qh = q.copy()
    qh[:, 0] += 3.0e5
    qh[:, 3] -= 7.0e6
    p = _abi.make_osc_params(6, kp=200)
    u, _ = be.osc(p, qh, dq, t)
    uo, _ = orc.osc(p, qh, dq, t)
    assert cases.rel_err(u, uo).max() <= 1e-6


def test_gpu_foreign_robot_config_runs_the_law_on_the_gpu():
    """OSC over a duck-typed robot_config that is NOT an abr_control_amd config (stand-in for the
    reference's MujocoConfig, arms/mujoco_config.py:201-451): its J/M/g/Tx/R/C are called per state
    like osc.py:242-301 does, the control law runs through abrk_osc_law_batch."""
    from abr_control_amd.controllers import OSC
    from oracle.oracle import Oracle

    class ForeignConfig:  # float32 casts like the reference's wrappers
        def __init__(self, arm):
            self.o = Oracle(_abi.load_table(arm))
            self.N_JOINTS = self.o.n

        def J(self, name, q, x=None):
            return self.o.J(name, q, x)

        def M(self, q):
            return self.o.M(q)

        def g(self, q):
            return self.o.g(q)

        def C(self, q, dq):
            return self.o.C(q, dq)

        def Tx(self, name, q, x=None):
            return self.o.Tx(name, q, x)

        def R(self, name, q):
            return self.o.R(name, q)

    class ForeignDamping:
        def __init__(self, rc, kv):
            self.rc, self.kv = rc, kv

        def generate(self, q, dq):
            return np.dot(self.rc.M(q), -self.kv * dq)

    g = golden("ur5")
    rc = ForeignConfig("ur5")
    for key, kw in (("cfg2", dict(kp=200)), ("cfg4", dict(kp=200, use_C=True)),
                    ("osc6_alg0", dict(kp=200, ko=150, kv=25, ctrlr_dof=[True] * 6, orientation_algorithm=0)),
                    ("osc_link5", dict(kp=200))):
        c = OSC(rc, **kw)
        gen = dict(ref_frame="link5") if key == "osc_link5" else {}
        u = c.generate(g[f"{key}_q"][:128], g[f"{key}_dq"][:128], g[f"{key}_target"][:128], **gen)
        assert cases.rel_err(u, g[f"{key}_uD"][:128]).max() <= 1e-6, key
        u1 = c.generate(g[f"{key}_q"][7], g[f"{key}_dq"][7], g[f"{key}_target"][7], **gen)
        assert u1.shape == (6,) and np.allclose(u1, u[7], rtol=1e-12, atol=1e-12)
        assert np.allclose(c.training_signal, g[f"{key}_tsD"][7], rtol=1e-9, atol=1e-9)
    g2 = golden("jaco2")
    rj = ForeignConfig("jaco2")
    c = OSC(rj, kp=200, null_controllers=[ForeignDamping(rj, 10)])
    u = c.generate(g2["cfg3_q"][:64], g2["cfg3_dq"][:64], g2["cfg3_target"][:64])
    assert cases.rel_err(u, g2["cfg3_uD"][:64]).max() <= 1e-6


def test_gpu_closed_loop_rollout_and_plant():
    """two-link plant step and the fused on-device control loop vs the reference's own loop
    (OSC.generate + ArmSim._step for 300 ms of simulated time, examples/PyGame/force_osc_xy.py:57-78)"""
    from abr_control_amd.arms import twojoint
    from abr_control_amd.controllers import OSC, Damping, RestingConfig

    g = golden("twojoint")
    T, every = int(g["rollout_T"]), int(g["rollout_every"])
    rc = twojoint.Config()
    mk = lambda: OSC(rc, kp=20, use_C=True, ctrlr_dof=[True, True, False, False, False, False], null_controllers=[
        Damping(rc, kv=10), RestingConfig(rc, kp=50, kv=np.sqrt(50), rest_angles=[np.pi / 4, np.pi])])
    # fused rollout, whole batch
    sim = twojoint.ArmSim(rc, dt=0.001, q_init=g["rollout_q0"].copy())
    sim.dq = g["rollout_dq0"].copy()
    qt, dqt, ut = sim.rollout(mk(), g["rollout_target"], T, every)
    assert np.max(np.abs(qt - g["rollout_qD"])) < 1e-9
    assert np.max(np.abs(dqt - g["rollout_dqD"])) < 1e-7
    assert np.max(np.abs(ut - g["rollout_uD"])) / np.max(np.abs(g["rollout_uD"])) < 1e-8
    assert np.array_equal(sim.q, qt[:, -1]) and abs(sim.t - 0.3) < 1e-12
    # the reference's own loop shape, one arm, step by step: generate -> send_forces
    sim1 = twojoint.ArmSim(rc, dt=0.001, q_init=g["rollout_q0"][5].copy())
    sim1.dq = g["rollout_dq0"][5].copy()
    c = mk()
    for t in range(50):
        fb = sim1.get_feedback()
        u = c.generate(q=fb["q"], dq=fb["dq"], target=g["rollout_target"][5])
        sim1.send_forces(u)
    assert sim1.q.shape == (2,)
    assert np.max(np.abs(sim1.q - g["rollout_qD"][5, 1])) < 1e-9  # checkpoint 2 = step 50
    # large batch: rollout == repeated single steps on the device (same bits), 4096 arms x 40 steps
    rng = np.random.RandomState(3)
    B = 4096
    q0 = np.array([np.pi / 4, np.pi / 4]) + rng.uniform(-0.6, 0.6, (B, 2))
    tgt = np.zeros((B, 6))
    tgt[:, :2] = rng.uniform(-1.5, 1.5, (B, 2))
    a = twojoint.ArmSim(rc, q_init=q0.copy())
    a.rollout(mk(), tgt, 40)
    b = twojoint.ArmSim(rc, q_init=q0.copy())
    c = mk()
    for t in range(40):
        b.send_forces(c.generate(b.q, b.dq, tgt))
    assert np.max(np.abs(a.q - b.q)) < 1e-12 and np.all(np.isfinite(a.q))
    with pytest.raises(Exception, match="two-link"):
        from abr_control_amd import engine
        from abr_control_amd.arms import ur5
        engine.osc_rollout_twolink(ur5.Config().arm_id, _abi.make_osc_params(6), a._plant, np.zeros((1, 2)),
                                   np.zeros((1, 2)), np.zeros((1, 6)), 1)


def test_gpu_launch_plan_equals_direct_call():
    import abr_control_amd as a
    from abr_control_amd import engine

    be = cases.GpuBackend("ur5")
    p = _abi.make_osc_params(6, kp=200, use_C=True, null_controllers=[_abi.make_damping(5)])
    q, dq, t = draw(31, 3000, 6)
    dq_, q_, t_ = a.DeviceArray.from_numpy(dq), a.DeviceArray.from_numpy(q), a.DeviceArray.from_numpy(t)
    u_ = a.DeviceArray((3000, 6))
    s = a.Stream(0)
    plan = engine.OscPlan(be.arm_id, 6, p, q_, dq_, t_, u_, stream=s)
    plan.launch()
    s.sync()
    ref, _ = be.osc(p, q, dq, t)
    assert np.array_equal(u_.numpy(), ref)
    # new state in the same buffers, relaunch
    q2, dq2, t2 = draw(32, 3000, 6)
    for d, h in ((q_, q2), (dq_, dq2), (t_, t2)):
        a._lib.check(a._lib.lib().abrk_memcpy_h2d(0, d.ptr, h.ctypes.data, h.nbytes, None))
    plan.launch()
    s.sync()
    assert np.array_equal(u_.numpy(), be.osc(p, q2, dq2, t2)[0])
    with pytest.raises(TypeError):
        engine.OscPlan(be.arm_id, 6, p, q, dq_, t_, u_)


def test_gpu_plan_graph_replay_equals_consecutive_launches():
    """abrk_plan_launch_graph(repeat) == `repeat` consecutive abrk_plan_launch calls, in order: with the integral
    term on (osc.py:262-264) every step reads the state its predecessor wrote, so a graph whose kernel nodes ran
    out of order or concurrently would change integrated_error and u."""
    import abr_control_amd as a
    from abr_control_amd import engine

    be = cases.GpuBackend("ur5")
    p = _abi.make_osc_params(6, kp=50, kv=7, ki=0.3)
    B = 4096
    q, dq, t = draw(41, B, 6)

    def run(graph):
        s = a.Stream(0)
        dev = [a.DeviceArray.from_numpy(x) for x in (q, dq, t)]
        ie, u = a.DeviceArray.from_numpy(np.zeros((B, 6))), a.DeviceArray((B, 6))
        plan = engine.OscPlan(be.arm_id, 6, p, dev[0], dev[1], dev[2], u, integrated_error=ie, stream=s)
        if graph:
            plan.launch_graph(5)
            plan.launch_graph(5)  # the cached executable graph, replayed
            plan.launch_graph(3)  # a different repeat count re-captures
        else:
            for _ in range(13):
                plan.launch()
        s.sync()
        return u.numpy(), ie.numpy()

    (ug, ieg), (ud, ied) = run(True), run(False)
    assert np.array_equal(ug, ud) and np.array_equal(ieg, ied)
    # and the state did advance: 13 steps of u_task accumulated (osc.py:263)
    ref = be.osc(p, q, dq, t, ie=np.zeros((B, 6)))[0]  # one step from a zero state
    assert not np.array_equal(ug, ref)
    from oracle.oracle import Oracle

    o = Oracle(_abi.load_table("ur5"))
    ie_o = np.zeros((B, 6))
    for _ in range(13):
        uo = o.osc_batch(p, q, dq, t, integrated_error=ie_o)
    assert cases.rel_err(ug, uo).max() < 1e-9 and np.abs(ieg - ie_o).max() < 1e-9


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7])
def test_gpu_user_arms_all_joint_counts(n):
    """runtime-table kernels for every joint count 1..ABRK_MAX_JOINTS on synthetic arms vs the oracle"""
    from abr_control_amd._abi import make_damping, make_osc_params as P
    from oracle.oracle import Oracle
    from tests.synthetic_arms import make_arm

    for nonorth in (False, True):
        tab = make_arm(n, 200 + n, nonorth)
        be, o = cases.GpuBackend(tab), Oracle(tab)
        rng = np.random.RandomState(n)
        B = 200
        q, dq, t = rng.uniform(-3, 3, (B, n)), rng.uniform(-2, 2, (B, n)), rng.uniform(-0.5, 0.5, (B, 6))
        r = be.dynamics(q, dq, "EE", [0.05, -0.02, 0.03], ("Tx", "J", "dJ", "M", "g", "C", "R", "quat"))
        for b in range(0, B, 9):
            assert np.allclose(r["Tx"][b], o.Tx("EE", q[b], [0.05, -0.02, 0.03]), atol=1e-12)
            assert np.allclose(r["J"][b], o.J("EE", q[b], [0.05, -0.02, 0.03]), atol=1e-12)
            assert np.allclose(r["dJ"][b], o.dJ("EE", q[b], dq[b], [0.05, -0.02, 0.03]), atol=1e-11)
            assert np.allclose(r["M"][b], o.M(q[b]), atol=1e-12) and np.allclose(r["g"][b], o.g(q[b]), atol=1e-12)
            assert np.allclose(r["C"][b], o.C(q[b], dq[b]), atol=1e-11)
            assert np.allclose(r["quat"][b], o.quaternion("EE", q[b]), atol=1e-10)
        k = min(n, 3)
        for p in (P(n, kp=30, ctrlr_dof=[1] * k + [0] * (6 - k)),
                  P(n, kp=30, ctrlr_dof=[1] * k + [0] * (6 - k), use_C=True, null_controllers=[make_damping(3)])):
            u, _ = be.osc(p, q, dq, t)
            uo = o.osc_batch(p, q, dq, t)
            ok = np.array([np.linalg.cond(o.M(q[b])) < 1e8 for b in range(B)])
            assert cases.rel_err(u, uo)[ok].max() < 1e-6


def test_gpu_inverse_kinematics():
    """InverseKinematics.generate_path, all three methods, against the reference's paths"""
    from abr_control_amd.arms import jaco2, ur5
    from abr_control_amd.controllers.path_planners import InverseKinematics

    for mod, arm in ((ur5, "ur5"), (jaco2, "jaco2")):
        g = golden(arm)
        ik = InverseKinematics(mod.Config())
        for method in (1, 2, 3):
            pp, vp = ik.generate_path(g["ik_q0"], g["ik_target"], n_timesteps=200, dt=0.001, method=method)
            assert pp.shape == (6, 200, 6)
            assert np.max(np.abs(pp - g[f"ik_m{method}_posD"])) < 1e-9
            assert np.max(np.abs(vp - g[f"ik_m{method}_velD"])) < 1e-9
        p1, v1 = ik.generate_path(g["ik_q0"][2], g["ik_target"][2])  # one path, reference shapes
        assert p1.shape == (200, 6) and np.allclose(p1, g["ik_m3_posD"][2], atol=1e-9)
        pos, vel = ik.next()
        assert pos.shape == (6,) and np.array_equal(pos, p1[0])
    # many paths at once: each row equals its own single-path run
    rng = np.random.RandomState(8)
    B = 5000
    q0 = rng.uniform(0.3, 2.8, (B, 6))
    rc = ur5.Config()
    tgt = np.hstack([rc.Tx("EE", q0 + rng.uniform(-0.5, 0.5, (B, 6))), rng.uniform(-1, 1, (B, 3))])
    ik = InverseKinematics(rc)
    pp, vp = ik.generate_path(q0, tgt, n_timesteps=100)
    assert np.all(np.isfinite(pp))
    p7, _ = ik.generate_path(q0[7], tgt[7], n_timesteps=100)
    assert np.array_equal(p7, pp[7])
    # the path makes progress towards the target position
    e0 = np.linalg.norm(rc.Tx("EE", q0) - tgt[:, :3], axis=1)
    e1 = np.linalg.norm(rc.Tx("EE", pp[:, -1]) - tgt[:, :3], axis=1)
    assert np.median(e1) < np.median(e0)


@pytest.mark.parametrize("variant", ["static", "rt"])
@pytest.mark.parametrize("arm", ARMS)
def test_gpu_secondary_controllers_match_reference(arm, variant):
    """AvoidJointLimits / Floating / AvoidObstacles kernels vs the reference's own outputs,
    alone and summed behind OSC's null-space filter"""
    g = golden(f"sec_{arm}")
    be = cases.GpuBackend(arm, variant)
    rep = cases.check_secondary_against_golden(be, arm, g)
    assert rep["obstacles_band"] <= 16
    cases.check_oscsec_against_golden(be, arm, g)


def test_gpu_secondary_controllers_large_batch_vs_oracle_and_api():
    """fresh seeded inputs vs the oracle; fp32; accumulate; DeviceArrays; the public classes inside OSC"""
    from abr_control_amd import DeviceArray
    from abr_control_amd.arms import ur5
    from abr_control_amd.controllers import OSC, AvoidJointLimits, AvoidObstacles, Damping, Floating
    from oracle.oracle import Oracle, avoid_joint_limits_batch

    g = golden("sec_ur5")
    tab = _abi.load_table("ur5")
    o = Oracle(tab)
    be = cases.GpuBackend("ur5")
    B = 3000
    q, dq, t = draw(11, B, 6)
    PL = cases.secondary_limit_params(g, "limB", 6)
    assert np.allclose(be.limits(PL, q), avoid_joint_limits_batch(6, PL, q), rtol=1e-13, atol=1e-13)  # exp() ulps
    for dyn, ts in ((0, 0), (1, 1)):
        uo, diag = o.floating_batch(dyn, ts, q[:600], dq[:600])
        ok = (np.abs(np.abs(diag[:, 0]) - 1e-3) > 1e-9) & (np.abs(diag[:, 1] - 1e-4) > 1e-8)
        assert cases.rel_err(be.floating(dyn, ts, q[:600], dq[:600]), uo)[ok].max() < 1e-9
    PO = cases.secondary_obstacle_params(g)
    uo, diag = o.avoid_obstacles_batch(PO, q[:600])
    ok = (diag[:, 0] > 1e-7) & (diag[:, 1] > 1e-20)
    ug = be.obstacles(PO, q)
    assert np.max(np.abs(ug[:600] - uo)[ok]) < 1e-6 * 500
    assert np.all(np.abs(ug) <= 500.0)  # np.clip(maximum), avoid_obstacles.py:121
    cases.check_secondary_against_golden(be, "ur5", g, dtype=np.float32)
    # public classes: single state, batch, device-resident, inside OSC
    rc = ur5.Config()
    ps = {k: g[f"limA_{k}"] for k in ("mn", "mx", "mt", "cz", "gr")}
    avoid = AvoidJointLimits(rc, list(ps["mn"]), list(ps["mx"]), list(ps["mt"]), list(ps["cz"]), list(ps["gr"]))
    assert np.allclose(avoid.generate(g["lim_q"][3], None), g["limA_u"][3], atol=1e-12)
    assert np.allclose(avoid.generate(g["lim_q"], None), g["limA_u"], atol=1e-12)
    obs = AvoidObstacles(rc, obstacles=g["obs_obstacles"], threshold=float(g["obs_threshold"]),
                         gain=float(g["obs_gain"]))
    fl = Floating(rc, dynamic=True, task_space=False)
    u1 = fl.generate(g["float_q"][0], g["float_dq"][0])
    assert u1.shape == (6,) and cases.rel_err(u1[None], g["float_d1t0_uD"][:1]).max() < 1e-9
    with pytest.raises(TypeError):
        fl.generate(g["float_q"][0])
    c = OSC(rc, kp=100, null_controllers=[avoid, obs, Damping(rc, 10)])
    qs, dqs, ts_ = g["oscsec_q"], g["oscsec_dq"], g["oscsec_target"]
    u = c.generate(qs, dqs, ts_)
    band = cases.threshold_band(g, "oscsec")
    _, diag = o.avoid_obstacles_batch(PO, qs)
    ok = ~band & (diag[:, 0] > 1e-7) & (diag[:, 1] > 1e-20)
    assert cases.rel_err(u, g["oscsec_uD"])[ok].max() < 1e-6
    qd, dqd, td = (DeviceArray.from_numpy(np.ascontiguousarray(a)) for a in (qs, dqs, ts_))
    ud = c.generate(qd, dqd, td)
    assert np.array_equal(ud.numpy(), u)
    # accumulate on device: u += signal
    base = DeviceArray.from_numpy(np.full((len(qs), 6), 0.5))
    obs._accumulate(qd, dqd, base)
    assert np.allclose(base.numpy() - 0.5, obs.generate(qs), atol=1e-9)


def test_gpu_concurrent_host_calls_from_threads():
    """ctypes releases the GIL: host-array calls from several threads (each with its own staging arenas,
    small batches through the pinned zero-copy arena, large ones through the copy engine) must not interfere"""
    from concurrent.futures import ThreadPoolExecutor

    be = cases.GpuBackend("ur5")
    params = cases.P(6, kp=200)

    def work(seed):
        out = []
        for k, B in enumerate((1, 37, 4096, 40000, 3)):
            q, dq, t = draw(100 * seed + k, B, 6)
            u, _ = be.osc(params, q, dq, t)
            out.append((q, dq, t, u))
        return out

    with ThreadPoolExecutor(4) as ex:
        results = list(ex.map(work, range(8)))
    for res in results:
        for q, dq, t, u in res:
            ref, _ = be.osc(params, q, dq, t)  # same call, single-threaded
            assert np.array_equal(u, ref)
    # and against the oracle on a sample
    from oracle.oracle import Oracle

    o = Oracle(_abi.load_table("ur5"))
    q, dq, t, u = results[3][1]
    uo, _ = o.osc_batch(params, q, dq, t, want_training=True)
    assert np.median(cases.rel_err(u, uo)) < 1e-9


def test_gpu_six_row_from_threads_on_default_stream():
    """VERDICT r2 / ADVICE: the six-row law's deferred pass (>= 16 384 rows) keeps a worklist per (device, stream); every
    Python call without an explicit stream is on the NULL stream and ctypes releases the GIL, so host threads share that
    worklist.  Memset, first pass and second pass of a call must enter the stream as a unit (abrk_host.cpp
    worklist_for): 8 threads, different batch sizes (so the buffer also grows under contention), orientation control,
    an integral state that only a completed row may update - bit-equal to the same calls made one after the other."""
    from concurrent.futures import ThreadPoolExecutor

    be = cases.GpuBackend("ur5")
    params = cases.P(6, kp=100, ko=80, kv=15, ki=0.2, ctrlr_dof=[1] * 6)
    sizes = (16384, 50000, 20001, 131072, 16385, 70000, 33333, 262144)

    def work(i):
        B = sizes[i]
        q, dq, t = draw(900 + i, B, 6)
        out = []
        for rep in range(3):
            ie = np.full((B, 6), 0.01 * rep)
            u, ts = be.osc(params, q, dq, t, ie=ie)
            out.append((u, ts, ie))
        return q, dq, t, out

    with ThreadPoolExecutor(8) as ex:
        results = list(ex.map(work, range(8)))
    for q, dq, t, out in results:
        for rep, (u, ts, ie) in enumerate(out):
            ie1 = np.full((len(q), 6), 0.01 * rep)
            u1, ts1 = be.osc(params, q, dq, t, ie=ie1)  # the same call, nobody else on the stream
            assert np.array_equal(u, u1) and np.array_equal(ts, ts1) and np.array_equal(ie, ie1)
            assert np.isfinite(u).all()
    # ... and right (4-5 % of random UR5 states take the truncating pinv with six task rows, i.e. the deferred pass)
    from oracle.oracle import Oracle

    q, dq, t, out = results[0]
    ie0 = np.zeros((2048, 6))
    uo, _ = Oracle(_abi.load_table("ur5")).osc_batch(params, q[:2048], dq[:2048], t[:2048], integrated_error=ie0,
                                                      want_training=True)
    err = cases.rel_err(out[0][0][:2048], uo)
    assert np.median(err) < 1e-9 and np.max(err) < 1e-6
    assert np.allclose(out[0][2][:2048], ie0, rtol=1e-12, atol=1e-12)


NOTS_CASES = [c for c in sorted(cases.CASES) if cases.takes_plain_six_row_law(c)]


@pytest.mark.parametrize("form", ["auto", "slices", "tiled", "recompute"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("variant", ["static", "rt"])
@pytest.mark.parametrize("case_id", NOTS_CASES)
def test_gpu_six_row_cases_without_training_signal(case_id, variant, dtype, form):
    """WHAT THE BENCH TIMES on the six-row law, and what any C-ABI caller without a training-signal buffer runs
    (include/abrk.h abrk_osc_generate_batch, training_signal = NULL): `osc_kernel<.., 6, .., FEAT = 0, PASS, NOTS = true>`
    in every pass (Launch::osc_launch) - gravity folded into the velocity term ahead of the factorisations.  Every golden
    case of the plain six-row law (UR5 six rows alg 0 / 1, vmax, orientation only, x-z-beta, link5; Jaco2 five and six
    rows; the three-joint arm's x-y-gamma) against the REFERENCE's outputs with no training signal asked for: built-in and
    runtime-table kernels, fp64 and fp32, and the four launch forms - "auto": first pass + finish kernel on hand-over
    records (`PASS = 1`); "slices": 48-row calls, the complete row program in one pass (`PASS = 0`, mode 0); "tiled":
    the rows repeated beyond 65 536, first pass + dense finish kernel on hand-over records (osc6_finish_dense_kernel);
    "recompute": the rows repeated beyond 1 M, first pass + recompute pass over the worklist (`PASS = 1`, then `PASS = 0`
    in mode 2).  Tiled forms: every repetition bit-equal.  Reference: controllers/osc.py:294-301,
    examples/timing_plots.py:36-37."""
    arm = cases.CASES[case_id]["arm"]
    be = cases.GpuBackend(arm, variant, training_signal=False, form=form)
    r = cases.check_case_against_golden(be, case_id, golden(arm), dtype=dtype)
    assert r["worst_vs_D"] <= (cases.TOL_F32 if dtype == np.float32 else
                               cases.TOL_THREEJOINT if arm == "threejoint" else cases.TOL_D)


@pytest.mark.parametrize("arm,variant", [("ur5", "static"), ("ur5", "rt"), ("jaco2", "static"), ("jaco2", "rt")])
def test_gpu_six_row_near_singular_postures_without_training_signal(arm, variant):
    """hundreds of truncating rows (postures next to the kinematic singularities) through the NOTS first pass and the
    finish kernel, against the oracle and against the same call WITH the training signal (1e-9: the two differ by where
    gravity joins the sum)"""
    be = cases.GpuBackend(arm, variant, training_signal=False)
    worst, n_trunc = cases.check_six_row_near_singular(be, arm, B=600, reference=cases.GpuBackend(arm, variant))
    assert n_trunc > 120 and worst <= cases.TOL_D


def test_gpu_fuzz_plain_six_row_law_without_training_signal():
    """random 1..7-joint user arms (runtime-table kernels), any mask / frame / offset / vmax / orientation algorithm, no
    optional input and no training signal - the NOTS kernels of every joint count against the oracle, hand-over form (96
    rows) and one-pass form (48-row slices)"""
    worst = 0.0
    for fc in cases.fuzz_osc_cases(61, 16, plain_six=True) + cases.fuzz_osc_cases(62, 16, plain_six=True):
        for form in ("auto", "slices"):
            worst = max(worst, cases.check_fuzz_case(lambda tab, f=form: cases.GpuBackend(tab, form=f), fc))
    assert worst < 1e-6


def test_gpu_compiled_arms_without_training_signal():
    """compiled user-arm plugins (specialize.py) carry their own NOTS instantiations: the three-joint plugin on the
    reference's x-y-gamma cases with no training signal (bit-equal to the built-in arm's kernels, and against the
    reference's outputs: hand-over, one-pass, dense-finish and recompute forms), the four-joint synthetic arm against the
    oracle - fp64 and fp32, hand-over and one-pass forms"""
    from oracle.oracle import Oracle
    from tests import compiled_arms

    arms_ = compiled_arms.test_arms()
    g = golden("threejoint")
    for form in ("auto", "slices", "tiled", "recompute"):
        cu = cases.GpuBackend(arms_["threejoint_user"], "compiled", training_signal=False, form=form)
        bi = cases.GpuBackend("threejoint", training_signal=False, form=form)
        for case_id in ("threejoint:osc_xyg_alg0", "threejoint:osc_xyg_alg1"):
            for dtype in (np.float64, np.float32):
                cases.check_case_against_golden(cu, case_id, g, dtype=dtype)
                a, _ = cases.run_case(cu, cases.CASES[case_id], g, dtype)
                b, _ = cases.run_case(bi, cases.CASES[case_id], g, dtype)
                assert np.array_equal(a, b), (case_id, dtype, form)
    tab = arms_["synthetic4"]
    o = Oracle(tab)
    rng = np.random.RandomState(5)
    B = 400
    q, dq, t = rng.uniform(-3, 3, (B, 4)), rng.uniform(-2, 2, (B, 4)), rng.uniform(-0.5, 0.5, (B, 6))
    ok = np.array([np.linalg.cond(o.M(q[b])) < 1e8 for b in range(B)])
    for kw in (dict(kp=30, ko=20, ctrlr_dof=[1, 1, 1, 1, 0, 0], vmax=[0.5, 1.0]),
               dict(kp=30, ko=20, kv=9, ctrlr_dof=[1, 0, 1, 0, 1, 1], use_C=True, orientation_algorithm=1)):
        p = _abi.make_osc_params(4, **kw)
        uo = o.osc_batch(p, q, dq, t)
        for form in ("auto", "slices"):
            u, ts = cases.GpuBackend(tab, "compiled", training_signal=False, form=form).osc(p, q, dq, t)
            assert ts is None and cases.rel_err(u, uo)[ok].max() < 1e-6, (kw, form)


def test_gpu_six_row_law_with_and_without_training_signal_agree():
    """the plain six-row law with no training signal asked for runs the NOTS instantiations in EVERY pass (round 5;
    `Launch::osc_launch`: first pass, recompute pass and the one-pass form alike): the same u as the call that asks for
    it, to rounding (gravity joins the sum at another place), deferred rows included - at 40 000 rows (hand-over), in
    8000-row calls, and in the one-pass form; UR5 and Jaco2, fp64"""
    for arm in ("ur5", "jaco2"):
        be = cases.GpuBackend(arm)
        for kw in (dict(kp=100, ko=60, kv=12, ctrlr_dof=[1] * 6),
                   dict(kp=100, ko=60, kv=12, ctrlr_dof=[1] * 6, use_C=True),
                   dict(kp=50, ctrlr_dof=[1, 1, 0, 1, 0, 1], use_g=False)):
            p = cases.P(6, **kw)
            q, dq, t = draw(77, 40000, 6)
            u_ts, _ = be.e.osc_generate(be.arm_id, 6, p, q, dq, t, training_signal=True)
            u_no = be.e.osc_generate(be.arm_id, 6, p, q, dq, t)
            assert np.isfinite(u_no).all()
            scale = np.max(np.abs(u_ts), axis=1, keepdims=True)
            # Jaco2's Mx_inv reaches cond 1e8: rounding-level differences are amplified by it
            tol = 1e-13 if arm == "ur5" else 1e-9
            assert np.max(np.abs(u_no - u_ts) / scale) < tol, (arm, kw)
            u_small = np.concatenate([be.e.osc_generate(be.arm_id, 6, p, q[lo:lo + 8000], dq[lo:lo + 8000],
                                                        t[lo:lo + 8000]) for lo in range(0, 40000, 8000)])
            assert np.array_equal(u_no, u_small), (arm, kw)  # bits do not depend on the batch a row arrives in
            u_one = np.concatenate([be.e.osc_generate(be.arm_id, 6, p, q[lo:lo + 48], dq[lo:lo + 48], t[lo:lo + 48])
                                    for lo in range(0, 960, 48)])
            assert np.array_equal(u_no[:960], u_one), (arm, kw)


def _bench_module():
    import importlib.util

    spec = importlib.util.spec_from_file_location("abrk_bench", os.path.join(os.path.dirname(__file__), "..", "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_BENCH_WORKLOADS = ["cfg1", "cfg2", "cfg3", "cfg4", "cfg5", "cfg2_f32", "dynF", "dynC", "oscF", "oscFC", "rollout", "ik",
                    "osc6", "osc5_j2", "sliding_j2", "joint", "limits", "floating", "obstacles"]


def test_gpu_bench_workload_list_is_complete():
    assert sorted(_BENCH_WORKLOADS) == sorted(_bench_module().WORKLOADS), "a bench workload without a parity test"


@pytest.mark.parametrize("workload", _BENCH_WORKLOADS)
def test_gpu_bench_workloads_match_the_oracle(workload):
    """TEST WHAT YOU TIME: every workload bench.py can print, built by bench.py's own `Runner` at 4096 rows - the same
    device buffers, the same optional arguments and NULLs, the same recorded plan `_enqueue` records (so the same kernel
    instantiation: no training-signal buffer -> the NOTS six-row kernels for `osc6` / `osc5_j2`) - stepped once through
    the plan, and its outputs compared with the CPU oracle on the same seeded rows.  A bench-only code path cannot go
    untested.  fp64: 1e-6 of the row's scale (north_star); fp32 workloads: 1e-4 on well-conditioned rows."""
    import abr_control_amd as a
    from oracle import oracle as orc

    bench = _bench_module()
    B = 4096
    st = a.Stream(0)
    if workload == "rollout":
        # the closed loop is sensitive to rounding where a target lies beyond the arm's reach (the arm stretches into its
        # singularity and rows hop between the branches of `_Mx`): 1000 steps amplify 1e-16 to 1e-2 on such rows.  The
        # same launch with 100 control steps per launch, compared on the rows whose target is reachable.
        bench.ROLLOUT_STEPS = 100
    r = bench.Runner(workload, B, 0, st)
    if r.kind == "rollout":
        q0, dq0, t6 = r.q.numpy().copy(), r.dq.numpy().copy(), r.t.numpy().copy()
    r.step()
    st.sync()
    q, dq, t = (np.asarray(x, float) for x in r.host)
    tab = _abi.load_table(r.arm)
    o = orc.Oracle(tab)
    n = r.n
    f32 = r.dt == np.float32
    tol = cases.TOL_F32 if f32 else cases.TOL_D
    kind = r.kind
    if kind in ("osc", "osc_damp", "osc_full"):
        p = r.params
        uo = o.osc_batch(p, q, dq, t)
        u = np.asarray(r.u.numpy(), float)
        dof = np.array(list(p.ctrlr_dof), bool)
        ok = np.ones(B, bool)
        cond = np.zeros(B)
        for b in range(B):
            J = o.J("EE", q[b], None)[dof]
            A = J @ np.linalg.inv(o.M(q[b])) @ J.T
            sv = np.linalg.svd(A, compute_uv=False)
            det = abs(np.linalg.det(A))
            cond[b] = sv.max() / max(sv.min(), 1e-300)
            near = abs(det - 1e-3) < 1e-8 or (det < 1.001e-3 and np.any(np.abs(sv / sv.max() - 1e-4) < 1e-8))
            ok[b] = not near and not (cond[b] > 1e9 and det >= 1e-3)
        if f32:
            ok &= cond < 1e3
        assert ok.sum() > (0.3 if f32 else 0.97) * B
        err = cases.rel_err(u, uo)
        assert np.isfinite(u).all() and err[ok].max() <= tol, f"{workload}: {err[ok].max():.3e} ({r.kernel_name()})"
        if kind == "osc_full":
            for w, arr in r.dyn_out.items():
                ref = np.array([{"Tx": lambda i: o.Tx("EE", q[i]), "J": lambda i: o.J("EE", q[i]), "M": lambda i: o.M(q[i]),
                                 "g": lambda i: o.g(q[i]), "C": lambda i: o.C(q[i], dq[i])}[w](i) for i in range(B)])
                assert np.max(np.abs(arr.numpy() - ref)) <= 1e-10 * max(np.max(np.abs(ref)), 1.0), (workload, w)
    elif kind == "dyn":
        ref = cases.OracleBackend(r.arm).dynamics(q, dq, "EE", None, tuple(r.want))
        for w in r.want:
            assert np.max(np.abs(r.dyn_out[w].numpy() - ref[w])) <= 1e-10 * max(np.max(np.abs(ref[w])), 1.0), (workload, w)
    elif kind == "sliding":
        uo, _ = o.sliding_batch(r.params, q, dq, t)
        u = np.asarray(r.u.numpy(), float)
        sv = np.array([np.linalg.svd(o.J("EE", q[b], None)[:3], compute_uv=False) for b in range(B)])
        rank = (sv > 1e-9 * sv.max(axis=1, keepdims=True)).sum(axis=1)
        smin = np.array([sv[b][rank[b] - 1] for b in range(B)])
        ok = (rank == rank.max()) & (sv.max(axis=1) / smin < (20 if f32 else 1e4))
        assert ok.sum() > 0.5 * B
        err = cases.rel_err(u, uo)
        assert np.isfinite(u).all() and err[ok].max() <= tol, f"{workload}: {err[ok].max():.3e}"
    elif kind == "joint":
        tj = np.asarray(r.tj.numpy(), float)
        uo = o.joint_batch(r.params, True, q, dq, tj, None)
        assert np.max(np.abs(r.u.numpy() - uo)) <= 1e-10 * np.max(np.abs(uo))
    elif kind == "limits":
        with np.errstate(all="ignore"):
            uo = orc.avoid_joint_limits_batch(n, r.params, q)
        assert np.allclose(r.u.numpy(), uo, rtol=1e-12, atol=1e-12)
    elif kind == "floating":
        uo, diag = o.floating_batch(int(r.params["dynamic"]), int(r.params["task_space"]), q, dq)
        ok = (np.abs(np.abs(diag[:, 0]) - 1e-3) > 1e-9) & (np.abs(diag[:, 1] - 1e-4) > 1e-8)
        assert cases.rel_err(np.asarray(r.u.numpy(), float), uo)[ok].max() <= tol
    elif kind == "obstacles":
        with np.errstate(all="ignore"):
            uo, diag = o.avoid_obstacles_batch(r.params, q)
        ok = (diag[:, 0] > 1e-7) & (diag[:, 1] > 1e-12)
        scale = np.maximum(np.max(np.abs(uo), axis=1), 1e-6)
        err = np.max(np.abs(r.u.numpy() - uo), axis=1) / scale
        assert ok.sum() > 0.9 * B and err[ok].max() <= 1e-5, err[ok].max()
    elif kind == "ik":
        rows = np.arange(0, B, 16)  # 200 iterations per path on the CPU: a sample of the 4096 paths
        pp, vp = orc.ik_paths(tab, r.params, q[rows], t[rows])
        assert np.max(np.abs(r.ik_out[0].numpy()[rows] - pp)) < 1e-8
        assert np.max(np.abs(r.ik_out[1].numpy()[rows] - vp)) < 1e-8
    elif kind == "rollout":
        qe, dqe, *_ = orc.rollout_twolink(tab, r.params, r.plant, q0, dq0, t6, bench.ROLLOUT_STEPS, bench.ROLLOUT_STEPS)
        qg, dqg = r.q.numpy(), r.dq.numpy()
        assert np.isfinite(qg).all()
        reach = np.linalg.norm(t6[:, :2], axis=1) < 1.5  # link lengths 1.0 + 0.6
        eq, edq = np.max(np.abs(qg - qe), axis=1), np.max(np.abs(dqg - dqe), axis=1)
        assert reach.sum() > 0.4 * B and eq[reach].max() < 1e-7 and edq[reach].max() < 1e-5, (eq[reach].max(), edq[reach].max())
        assert np.percentile(eq, 90) < 1e-7, np.percentile(eq, 90)
    else:
        raise AssertionError(f"no oracle comparison for bench workload kind {kind!r}")
    if r.plan is not None:
        r.plan.close()


def test_gpu_bench_dumps_what_the_timed_path_computed(tmp_path):
    """`bench.py --gpus 1 --steps K --dump-outputs DIR`: the line reports the K timed steps and their ms_per_step, and
    DIR/u.npy is bit-equal to one step of the same recorded plan on the same seeded inputs"""
    import json
    import subprocess
    import sys

    import abr_control_amd as a
    from tests.conftest import REPO

    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "3",
           "--dump-outputs", str(tmp_path), "--no-roofline-leg", "--no-strong-leg", "--no-cpu-baseline"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 30 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 4096) < 1e-3 * 4096  # value = rows x steps / (steps x ms_per_step)
    assert sorted(os.listdir(tmp_path)) == ["u.npy"]
    bench = _bench_module()
    st = a.Stream(0)
    r = bench.Runner("cfg2", 4096, 0, st)
    r.step()
    st.sync()
    u = np.load(tmp_path / "u.npy")
    assert u.dtype == np.float64 and np.array_equal(u, r.u.numpy())
    r.plan.close()


@pytest.mark.parametrize("launcher", ["self", "external"])
def test_gpu_bench_two_ranks_share_one_device(tmp_path, launcher):
    """the N > 1 launch contract on a one-GPU box: plain `python bench.py --gpus 2` (the command launches its own ranks;
    VERDICT r4 #1) and the same command under an external one-process-per-GPU launcher (`torch.distributed.run`), both
    ranks on device 0 behind the explicit --allow-shared-device test flag: ONE contract line with n_gpus = 2, the
    strong-scaling leg cuts BASELINE config 4's 2^20 rows into two contiguous shards, and each rank's shard of u is
    bit-equal to the same rows of the unsharded call.  Without the flag the run refuses to double up."""
    import hashlib
    import json
    import subprocess
    import sys

    import abr_control_amd as a
    from tests.conftest import REPO

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["MASTER_ADDR"] = "127.0.0.1"
    bench_args = ["--gpus", "2", "--steps", "100", "--warmup", "10", "--roofline-batch", "262144", "--roofline-steps",
                  "5", "--sustain-seconds", "0.2", "--dump-shard-u", str(tmp_path)]
    if launcher == "self":
        cmd = [sys.executable, os.path.join(REPO, "bench.py")] + bench_args
        if a.device_count() < 2:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
            assert p.returncode == 1 and json.loads(p.stdout.strip())["devices_seen"] == a.device_count()
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", "29533", os.path.join(REPO, "bench.py")] + bench_args
    p = subprocess.run(cmd + ["--allow-shared-device"], capture_output=True, text=True, timeout=900, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["steps"] == 100 and d["value"] > 1e6
    assert d["n_ranks_seen"] == 2 and [r["rank"] for r in d["ranks"]] == [0, 1]
    assert d["shared_device"] == (a.device_count() < 2)
    assert d["config"]["global_batch"] == 2 * 4096 and "cpu_baseline" not in d
    s4 = d["strong_scaling_cfg4"]
    assert s4["n_gpus"] == 2 and s4["rows_per_gpu"] == 1 << 19 and s4["global_batch"] == 1 << 20 and s4["scaling"] == "strong"
    assert s4["n_ranks_seen"] == 2
    per = d["roofline_per_gpu"]
    assert per["n_ranks_seen"] == 2 and [g["rank"] for g in per["gpus"]] == [0, 1] and all(0 < g["frac"] < 1 for g in per["gpus"])
    assert 0 < d["roofline"]["frac"] < 1 and d["roofline"]["sustained"]["seconds"] >= 0.15  # (the run is sized from a 5-launch estimate: about the 0.2 s asked for)
    # the shards: rows [0, 2^19) and [2^19, 2^20) of the one seeded global batch, against the unsharded call
    import bench

    be = cases.GpuBackend("ur5")
    q, dq, t = bench.make_inputs(1, 1 << 20, 6, 6, np.float64)
    u, _ = be.osc(cases.P(6, kp=200, use_g=True, use_C=True), q, dq, t)
    for r in (0, 1):
        sh = json.load(open(tmp_path / f"shard_u_rank{r}.json"))
        assert (sh["lo"], sh["hi"]) == (r << 19, (r + 1) << 19)
        assert sh["sha256"] == hashlib.sha256(np.ascontiguousarray(u[sh["lo"]:sh["hi"]]).tobytes()).hexdigest()


def test_gpu_bench_single_process_drives_every_shard():
    """`bench.py --gpus N --single-process`: one process, one host thread, N resident shards (here all on device 0 -
    --allow-shared-device): the line carries value / strong_scaling_cfg4 / resident_shard_step_cfg4 with n_devices_seen,
    and refuses to double up without the test flag"""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--single-process", "--steps", "20", "--warmup", "5"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 1 and d["devices_seen"] == 1 and "error" in d
    r = subprocess.run(cmd + ["--allow-shared-device"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 2 and d["n_devices_seen"] == 1 and d["devices"] == [0, 0] and d["shared_device"]
    assert d["value"] > 1e8 and d["strong_scaling_cfg4"]["rows_per_gpu"] == (1 << 19)
    rs = d["resident_shard_step_cfg4"]
    assert rs["shards"] == 8 and rs["rows_per_shard"] == 131072
    # VERDICT r5 "Next" #3: the resident 8-shard step of config 4 costs at most 1.3 x eight plain 131 072-row launches
    assert rs["ratio_to_eight_plain_launches"] <= 1.3, rs


def test_gpu_merged_loops_equal_separate_loops():
    """VERDICT r5 "Next" #7 (independent control loops stop overlapping beyond two streams): engine.MergedLoops puts the
    loops' rows into one batch - every loop writes / reads DeviceArray views of shared buffers, one launch per tick
    evaluates all of them.  Each loop's torques are bit-equal to its own separate call (x,y,z law with integral state
    over 4 ticks; six-row law), loops of unequal size."""
    import abr_control_amd as a
    from abr_control_amd import engine

    be = cases.GpuBackend("ur5")
    rows = [4096, 1000, 64, 4096, 7, 2500]
    data = [draw(200 + i, r, 6) for i, r in enumerate(rows)]
    for kw in (dict(kp=100, kv=15, ki=0.2, use_C=True), dict(kp=200, ko=150, kv=25, ctrlr_dof=[1] * 6)):
        p = _abi.make_osc_params(6, **kw)
        loops = engine.MergedLoops(be.arm_id, 6, p, rows, training_signal=True)
        for i, (q, dq, t) in enumerate(data):
            v = loops.loop(i)
            v.q.copy_from_numpy(q), v.dq.copy_from_numpy(dq), v.target.copy_from_numpy(t)
        ies = [np.zeros((r, 6)) for r in rows]
        for tick in range(4):
            if tick % 2:
                loops.launch_graph(1)
            else:
                loops.launch()
            loops.stream.sync()
            for i, (q, dq, t) in enumerate(data):
                u0, ts0 = be.e.osc_generate(be.arm_id, 6, p, q, dq, t, None, ies[i] if p.ki else None, training_signal=True)
                v = loops.loop(i)
                assert np.array_equal(v.u.numpy(loops.stream), u0), (kw, tick, i)
                assert np.array_equal(v.training_signal.numpy(loops.stream), ts0), (kw, tick, i)
                if p.ki:
                    assert np.array_equal(v.integrated_error.numpy(loops.stream), ies[i])
        loops.close()
    d = a.DeviceArray.from_numpy(np.arange(40.0).reshape(10, 4))
    assert np.array_equal(d.rows(3, 7).numpy(), np.arange(40.0).reshape(10, 4)[3:7])
    with pytest.raises(IndexError):
        d.rows(5, 11)


def test_gpu_secondary_controllers_properties_full_size():
    """size-independent properties at 2^20 rows (BASELINE config-4 size)"""
    be = cases.GpuBackend("ur5")
    B = 1 << 20
    q, dq, _ = draw(21, B, 6)
    # Floating(joint space) == -g of the dynamics kernel; dynamic adds -M dq (floating.py:64-69)
    d = be.dynamics(q[:65536], None, "EE", None, ("g", "M"))
    u = be.floating(0, 0, q, dq)
    assert u.shape == (B, 6) and np.allclose(u[:65536], -d["g"], rtol=1e-13, atol=1e-13)
    ud = be.floating(1, 0, q[:65536], dq[:65536])
    assert np.allclose(ud, -d["g"] - np.einsum("bij,bj->bi", d["M"], dq[:65536]), rtol=1e-12, atol=1e-12)
    # task space: u = J^T u_task lies in the row space of J[:3]: projecting it through pinv(J) J changes nothing
    ut = be.floating(0, 1, q[:4096], dq[:4096])
    J = be.dynamics(q[:4096], None, "EE", None, ("J",))["J"][:, :3]
    res = ut - np.einsum("bij,bj->bi", np.linalg.pinv(J) @ J, ut)
    assert np.max(np.abs(res)) < 1e-8 * max(1.0, np.max(np.abs(ut)))
    # joint limits: walls only -> every entry is 0 or +-max_torque, 0 strictly inside the range
    PL = _abi.make_limits_params(6, [1.0] * 6, [5.0] * 6, max_torque=[3.0] * 6)
    ul = be.limits(PL, q)
    assert set(np.unique(ul)) <= {-3.0, 0.0, 3.0}
    assert np.array_equal(ul != 0, (q < 1.0) | (q > 5.0))
    assert np.array_equal(ul > 0, q < 1.0)
    # obstacles: none / out of reach -> exactly 0; always within +-maximum; rows independent of batch position
    assert not be.obstacles(_abi.make_obstacles_params([]), q[:4096]).any()
    assert not be.obstacles(_abi.make_obstacles_params([[50.0, 50.0, 50.0, 0.1]]), q[:4096]).any()
    PO = _abi.make_obstacles_params([[0.3, 0.2, 0.4, 0.1], [-0.2, 0.4, 0.3, 0.05]], threshold=0.3, gain=30,
                                    maximum=123.0)
    uo = be.obstacles(PO, q)
    assert np.all(np.isfinite(uo)) and np.max(np.abs(uo)) <= 123.0 and (uo != 0).any()
    perm = np.random.RandomState(5).permutation(B)[:8192]
    assert np.array_equal(be.obstacles(PO, q[perm]), uo[perm])


def test_gpu_fuzz_osc_parameter_space():
    """seeded random controller configurations (ctrlr_dof masks, frames, offsets, vmax, ki, target velocity,
    fused + external secondary controllers, both orientation algorithms) on random 1..7-joint user arms"""
    worst = 0.0
    for fc in cases.fuzz_osc_cases(7, 24) + cases.fuzz_osc_cases(8, 24):
        worst = max(worst, cases.check_fuzz_case(cases.GpuBackend, fc))
    assert worst < 1e-6


@pytest.mark.parametrize("arm", ["twojoint", "threejoint"])
def test_gpu_xy_fast_kernel_equals_general_kernel(arm):
    """x,y control on arms of <= 3 joints runs the two-row kernel; a zero external null signal forces the masked
    six-row kernel on the same inputs"""
    for variant in ("static", "rt"):
        be = cases.GpuBackend(arm, variant)
        n = be.n
        rng = np.random.RandomState(3)
        B = 3000
        q, dq, t = rng.uniform(0, 6.28, (B, n)), rng.uniform(-3, 3, (B, n)), rng.uniform(-1, 1, (B, 6))
        for kw in (dict(kp=20, kv=5), dict(kp=20, kv=5, vmax=[0.5, 0.5], use_C=True, xyz_offset=[0.1, -0.05, 0.0]),
                   dict(kp=30, ki=0.2, null_controllers=[cases.make_damping(4)])):
            p = cases.P(n, ctrlr_dof=cases.XY, **kw)
            ie1 = np.zeros((B, 6)) if kw.get("ki") else None
            ie2 = np.zeros((B, 6)) if kw.get("ki") else None
            u1, ts1 = be.osc(p, q, dq, t, ie=ie1)
            u2, ts2 = be.osc(p, q, dq, t, ie=ie2, une=np.zeros((B, n)))
            assert np.allclose(u1, u2, rtol=1e-10, atol=1e-10) and np.allclose(ts1, ts2, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("arm", ["ur5", "threejoint"])
def test_gpu_six_row_use_C_on_orthogonal_chains(arm):
    """orientation / arbitrary-row control with Coriolis compensation on built-in arms (two-pass kernels)"""
    assert cases.check_six_row_use_C(cases.GpuBackend(arm), arm, B=2000) < 1e-6


def test_gpu_fuzz_sliding_joint_dynamics():
    """Sliding / Joint / Damping / RestingConfig / every robot_config output on random 1..7-joint user arms"""
    for seed in range(16):
        cases.check_fuzz_other(cases.GpuBackend, seed)


# ---- the reference's own tests of the OSC helper methods (controllers/tests/test_osc.py), through the Python
# mirror -> C ABI -> kernels, against the reference's outputs (tests/golden/oschelpers_<arm>.npz) and the oracle
HELPER_ARMS = ["ur5", "jaco2", "threejoint"]


def _arm_config(arm):
    import importlib

    return importlib.import_module(f"abr_control_amd.arms.{arm}").Config()


@pytest.mark.parametrize("arm", HELPER_ARMS)
def test_gpu_velocity_limiting(arm):
    """test_osc.py:12-59, same gains, inputs and expected values"""
    from abr_control_amd.controllers import OSC

    g = golden(f"oschelpers_{arm}")
    robot_config = _arm_config(arm)
    kp, ko, kv, vmax = 10, 8, 4, 1
    ctrlr = OSC(robot_config, kp=kp, ko=ko, kv=kv, ctrlr_dof=[True] * 6, vmax=[vmax, vmax])
    answer = [kp * 0.05] * 3 + [ko * 0.05] * 3
    assert np.allclose(ctrlr._velocity_limiting(np.ones(6) * 0.05), answer, atol=1e-5)
    u_task = np.hstack([np.ones(3) * 100, np.ones(3) * 0.05])
    answer = [kv * np.sqrt(vmax / 3.0)] * 3 + [ko * 0.05] * 3
    assert np.allclose(ctrlr._velocity_limiting(u_task), answer, atol=1e-5)
    answer = [kv * np.sqrt(vmax / 3.0)] * 6
    assert np.allclose(ctrlr._velocity_limiting(np.ones(6) * 100), answer, atol=1e-5)
    # the reference's own outputs, as one batch
    got = ctrlr._velocity_limiting(g["vl_in"])
    assert np.max(np.abs(got - g["vl_out"])) < 1e-12


@pytest.mark.parametrize("arm", HELPER_ARMS)
def test_gpu_Mx(arm):
    """test_osc.py:62-86 (J = I => Mx = M with threshold 1e-5; J = ones => rank one), then the reference's outputs
    on random task rows"""
    from abr_control_amd.controllers import OSC
    from oracle import oracle as O

    g = golden(f"oschelpers_{arm}")
    robot_config = _arm_config(arm)
    n = robot_config.N_JOINTS
    ctrlr = OSC(robot_config, ctrlr_dof=[True] * min(n, 6) + [False] * (6 - min(n, 6)))
    rng = np.random.RandomState(5)
    for ii in range(20):
        q = rng.random_sample(n) * 2 * np.pi
        J = np.eye(n)
        M = robot_config.M(q=q)
        Mx, M_inv = ctrlr._Mx(M=M, J=J, threshold=1e-5)
        assert np.allclose(M, Mx, atol=1e-5)
        assert np.allclose(M_inv @ M, np.eye(n), atol=1e-4)  # M is float32-rounded (base_config.py:285)
        J = np.ones((6, n))
        Mx, M_inv = ctrlr._Mx(M=M, J=J)
        U2, S2, Vh2 = np.linalg.svd(Mx)
        assert np.all(np.abs(S2[1:]) < 1e-10)
    # batched, against the reference's outputs
    M = g["mx_M"]
    B = M.shape[0]
    Mx, Minv = ctrlr._Mx(M, np.broadcast_to(np.eye(n), (B, n, n)).copy(), threshold=1e-5)
    assert np.max(np.abs(Mx - g["mx_eye_Mx"]) / np.abs(g["mx_eye_Mx"]).max(axis=(1, 2), keepdims=True)) < 1e-9
    assert np.max(np.abs(Minv - g["mx_eye_Minv"]) / np.abs(g["mx_eye_Minv"]).max(axis=(1, 2), keepdims=True)) < 1e-9
    Mx1, _ = ctrlr._Mx(M, np.ones((B, 6, n)))
    assert np.max(np.abs(Mx1 - g["mx_ones_Mx"]) / np.abs(g["mx_ones_Mx"]).max(axis=(1, 2), keepdims=True)) < 1e-9
    for k in (1, 2, 3, 6):
        if f"mx_k{k}_J" not in g.files:
            continue
        ok = cases.mx_rows_clear_of_thresholds(g[f"mx_k{k}_det"], g[f"mx_k{k}_sv"])
        Mxk, _ = ctrlr._Mx(M, g[f"mx_k{k}_J"])
        ref = g[f"mx_k{k}_Mx"]
        scale = np.maximum(np.abs(ref).max(axis=(1, 2)), 1e-300)
        err = np.abs(Mxk - ref).max(axis=(1, 2)) / scale
        assert err[ok].max() <= 1e-7, (arm, k, err[ok].max())
        # and the oracle on the same rows (incl. the rows the band test sets aside for the reference comparison)
        orc = np.array([O.osc_mx(M[b], g[f"mx_k{k}_J"][b])[0] for b in range(B)])
        erro = np.abs(Mxk - orc).max(axis=(1, 2)) / np.maximum(np.abs(orc).max(axis=(1, 2)), 1e-300)
        assert erro[ok].max() <= 1e-7


@pytest.mark.parametrize("alg", [0, 1])
@pytest.mark.parametrize("arm", HELPER_ARMS)
def test_gpu_calc_orientation_forces(arm, alg):
    """test_osc.py:94-140, called with the ref_frame argument the method requires (the reference's test omits it and
    fails): the error quaternion's distance to the target shrinks after a small step along the
    returned direction; and equality with the reference's own outputs"""
    from abr_control_amd.controllers import OSC
    from oracle import oracle as O

    g = golden(f"oschelpers_{arm}")
    robot_config = _arm_config(arm)
    ctrlr = OSC(robot_config, orientation_algorithm=alg, ctrlr_dof=[True] * 6)
    got = ctrlr._calc_orientation_forces(g["of_abg"], g["of_q"], "EE")
    assert got.shape == (len(g["of_q"]), 3)
    tol = 2e-5 if arm == "threejoint" else 1e-9  # threejoint: the reference's float32 link lengths (tests/cases.py)
    assert np.max(np.abs(got - g[f"of_alg{alg}"])) < tol
    one = ctrlr._calc_orientation_forces(g["of_abg"][3], g["of_q"][3], "EE")
    assert one.shape == (3,) and np.array_equal(one, got[3])
    # from the reference's own rotation matrices: the law alone
    from abr_control_amd import engine

    direct = engine.osc_orientation_forces(alg, g["of_R"], g["of_abg"])
    assert np.max(np.abs(direct - g[f"of_alg{alg}"])) < 1e-9
    orc = np.array([O.osc_orientation_forces(alg, R, a) for R, a in zip(g["of_R"], g["of_abg"])])
    assert np.max(np.abs(direct - orc)) < 1e-9


def test_gpu_osc_helpers_fp32_and_errors():
    """the float32 instantiations of the three helper kernels, and the argument checks of their entry points"""
    from abr_control_amd import engine
    from abr_control_amd._lib import AbrkError

    g = golden("oschelpers_ur5")
    kp, ko, kv, v0, v1 = g["vl_gains"]
    p = _abi.make_osc_params(6, kp=kp, ko=ko, kv=kv, vmax=[v0, v1], ctrlr_dof=[1] * 6)
    f32 = np.float32
    got = engine.osc_velocity_limiting(p, g["vl_in"].astype(f32), dtype=f32)
    assert got.dtype == f32 and np.max(np.abs(got - g["vl_out"])) < 1e-4
    for alg in (0, 1):
        got = engine.osc_orientation_forces(alg, g["of_R"].astype(f32), g["of_abg"].astype(f32), dtype=f32)
        assert np.max(np.abs(got - g[f"of_alg{alg}"])) < 1e-4
    B, n = g["mx_M"].shape[:2]
    Mx, Minv = engine.osc_mx(n, g["mx_M"].astype(f32), np.broadcast_to(np.eye(n, dtype=f32), (B, n, n)).copy(), 1e-5,
                             dtype=f32)
    assert np.max(np.abs(Mx - g["mx_eye_Mx"]) / np.abs(g["mx_eye_Mx"]).max(axis=(1, 2), keepdims=True)) < 2e-3
    # argument checks
    with pytest.raises(AbrkError, match="vmax"):
        engine.osc_velocity_limiting(_abi.make_osc_params(6, kp=10), g["vl_in"])
    with pytest.raises(AbrkError, match="Invalid algorithm number"):
        engine.osc_orientation_forces(2, g["of_R"], g["of_abg"])
    with pytest.raises(AbrkError, match="task rows"):
        engine.osc_mx(n, g["mx_M"], np.ones((B, 7, n)))
    # empty batch
    Mx, _ = engine.osc_mx(n, np.zeros((0, n, n)), np.zeros((0, 3, n)))
    assert Mx.shape == (0, 3, 3)


def test_gpu_twojoint_closed_forms_through_robot_config():
    """abr_control/arms/tests/test_base_config.py:40-180 (test_g, test_dJ, test_J, test_M, test_R, test_C, test_Tx,
    test_T_inv): every robot_config function of the two-link arm against the hand-derived closed forms of the
    reference's fixture (arms/tests/dummy_base_arm.py) on its grids, np.allclose defaults as there - here through the
    Python mirror, whole grids per call"""
    from abr_control_amd.arms import twojoint

    k = golden("known_answers")
    robot_config = twojoint.Config()
    Q, QD = k["q_grid"], k["qdq_grid"]
    assert np.allclose(robot_config.g(Q), k["g"])
    assert np.allclose(robot_config.M(Q), k["M"])
    assert np.allclose(robot_config.C(QD[:, :2], QD[:, 2:]), k["C"])
    for name in ("link0", "joint0", "link1", "joint1", "link2", "EE"):
        assert np.allclose(robot_config.J(name, Q), k[f"J_{name}"]), name
        assert np.allclose(robot_config.dJ(name, QD[:, :2], QD[:, 2:]), k[f"dJ_{name}"]), name
        assert np.allclose(robot_config.R(name, Q), k[f"R_{name}"]), name
        assert np.allclose(robot_config.Tx(name, Q), k[f"Tx_{name}"]), name
        assert np.allclose(robot_config.T_inv(name, Q), k[f"Tinv_{name}"]), name
    # one state at a time, as the reference's tests call them: reference shapes and dtypes (base_config.py:223-415)
    q, dq = Q[77], QD[1234, 2:]
    assert robot_config.g(q).shape == (2,) and robot_config.g(q).dtype == np.float32
    assert robot_config.M(q).shape == (2, 2) and robot_config.J("EE", q).shape == (6, 2)
    assert robot_config.Tx("EE", q).dtype == np.float64 and robot_config.Tx("EE", q).shape == (3,)
    assert robot_config.C(q, dq).shape == (2, 2) and robot_config.dJ("EE", q, dq).shape == (6, 2)
    with pytest.raises(Exception, match="Invalid transformation name"):
        robot_config.Tx("link9", q)


def test_gpu_transformations_known_answers():
    """abr_control/utils/transformations.py: the six functions on the control path against the reference's own
    outputs on seeded inputs (tests/golden/known_answers.npz, written by oracle/gen_golden.py) and its doctest
    constants (:1203-1214, :1276-1277, :1295-1299)"""
    from abr_control_amd.utils import transformations as tf

    k = golden("known_answers")
    ang = k["tf_angles"]
    assert np.allclose(tf.quaternion_from_euler(ang[:, 0], ang[:, 1], ang[:, 2], "rxyz"), k["tf_quat_from_euler_rxyz"],
                       atol=1e-14)
    M = tf.euler_matrix(ang[:, 0], ang[:, 1], ang[:, 2], "rxyz")
    assert M.shape == (len(ang), 4, 4) and np.allclose(M[:, :3, :3], k["tf_euler_matrix_rxyz"], atol=1e-14)
    assert np.allclose(M[:, 3], [0, 0, 0, 1]) and np.allclose(M[:, :3, 3], 0)
    assert np.allclose(tf.quaternion_from_matrix(k["tf_euler_matrix_rxyz"]), k["tf_quat_from_matrix"], atol=1e-12)
    assert np.allclose(tf.quaternion_multiply(k["tf_qa"], k["tf_qb"]), k["tf_quat_mul"], atol=1e-14)
    assert np.allclose(tf.quaternion_conjugate(k["tf_qa"]), k["tf_quat_conj"], atol=0)
    assert np.allclose(tf.unit_vector(k["tf_qa"], axis=-1), k["tf_unit"], atol=1e-15)
    # the reference's doctests
    assert np.allclose(tf.quaternion_multiply([4, 1, -2, 3], [8, -5, 6, 7]), [28, -44, -14, 48])
    assert np.allclose(tf.quaternion_from_matrix(np.identity(4), True), [1, 0, 0, 0])
    R = [[-0.545, 0.797, 0.260, 0], [0.733, 0.603, -0.313, 0], [-0.407, 0.021, -0.913, 0], [0, 0, 0, 1]]
    assert np.allclose(tf.quaternion_from_matrix(R), [0.19069, 0.43736, 0.87485, -0.083611], atol=1e-5)
    R = [[0.395, 0.362, 0.843, 0], [-0.626, 0.796, -0.056, 0], [-0.677, -0.498, 0.529, 0], [0, 0, 0, 1]]
    assert np.allclose(tf.quaternion_from_matrix(R), [0.82336615, -0.13610694, 0.46344705, -0.29792603], atol=1e-5)
    q0 = k["tf_qa"][0]
    q1 = tf.quaternion_conjugate(q0)
    assert q1[0] == q0[0] and all(q1[1:] == -q0[1:])
    v0 = np.array([0.3, -1.2, 2.0])
    assert np.allclose(tf.unit_vector(v0), v0 / np.linalg.norm(v0))
    # the default axes of the reference ('sxyz') against the closed form of transformations.py:1131-1147
    ai, aj, ak = 0.3, -0.7, 1.9
    ci, si, cj, sj, ck, sk = (f(x / 2) for x in (ai, aj, ak) for f in (np.cos, np.sin))
    want = [cj * ci * ck + sj * si * sk, cj * si * ck - sj * ci * sk, cj * si * sk + sj * ci * ck,
            cj * ci * sk - sj * si * ck]
    assert np.allclose(tf.quaternion_from_euler(ai, aj, ak), want, atol=1e-15)
    with pytest.raises(ValueError):
        tf.quaternion_from_euler(1, 2, 3, "ryxz")


def test_gpu_sliding_plan_equals_direct_call():
    """abrk_sliding_plan_create + abrk_plan_launch / abrk_plan_launch_graph == abrk_sliding_generate_batch"""
    import abr_control_amd as a
    from abr_control_amd import engine

    be = cases.GpuBackend("threejoint")
    p = _abi.make_sliding_params(3)
    B = 5000
    q, dq, t = draw(51, B, 3, nt=3)
    ref_u, ref_s = be.sliding(p, q, dq, t)
    s = a.Stream(0)
    dev = [a.DeviceArray.from_numpy(x) for x in (q, dq, t)]
    u_, s_ = a.DeviceArray((B, 3)), a.DeviceArray((B, 3))
    plan = engine.SlidingPlan(be.arm_id, 3, p, dev[0], dev[1], dev[2], u_, s=s_, stream=s)
    plan.launch()
    s.sync()
    assert np.array_equal(u_.numpy(), ref_u) and np.array_equal(s_.numpy(), ref_s)
    a._lib.check(a._lib.lib().abrk_memset(0, u_.ptr, 0, u_.nbytes, None))
    plan.launch_graph(7)
    s.sync()
    assert np.array_equal(u_.numpy(), ref_u)
    with pytest.raises(TypeError):
        engine.SlidingPlan(be.arm_id, 3, p, q, dev[1], dev[2], u_)


def test_gpu_fuzz_secondary_controllers():
    """AvoidJointLimits / Floating / AvoidObstacles on random user arms with random parameters vs the oracle"""
    for seed in range(20, 60):
        cases.check_fuzz_secondary(cases.GpuBackend, seed)


def test_gpu_examples_run_from_a_checkout():
    """the headless example loops (the reference's PyGame scripts with the interface taken out) run as scripts"""
    import glob
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scripts = sorted(glob.glob(os.path.join(root, "examples", "*.py")))
    assert len(scripts) >= 3
    for sc in scripts:
        r = subprocess.run([sys.executable, sc], cwd="/tmp", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"{sc}:\n{r.stderr[-800:]}"


def test_gpu_truncated_pinv_rows_are_compared():
    """every golden row on which `pinv(Mx_inv, rcond=1e-4)` really truncates (osc.py:142-145; 49 rows over the OSC
    cases) takes part in the golden assert - only rows within 1e-6 (relative) of a threshold may be excluded"""
    tot = cmp_ = 0
    for case_id, case in sorted(cases.CASES.items()):
        if case["kind"] != "osc":
            continue
        r = cases.check_case_against_golden(cases.GpuBackend(case["arm"], "static"), case_id, golden(case["arm"]))
        tot += r["n_trunc"]
        cmp_ += r["n_trunc_compared"]
        assert r["n_band"] <= 1, (case_id, r)
    assert tot >= 45 and cmp_ == tot, (tot, cmp_)


@pytest.mark.parametrize("arm", ["ur5", "jaco2"])
def test_gpu_quaternion_every_frame(arm):
    """power-iteration quaternion vs the reference's eigh on every frame, incl. Jaco2's non-orthogonal late frames"""
    cases.check_quaternions_all_frames(cases.GpuBackend(arm, "static"), arm, golden(f"quat_{arm}"))


# ---------------------------------------------------------------------------- recorded launch plans (abrk_plan_begin/end)
def _dev(*arrays):
    import abr_control_amd as a

    return [a.DeviceArray.from_numpy(np.ascontiguousarray(x)) for x in arrays]


def _zero(arr):
    """memset on the null stream, completed before anything is enqueued on the (non-blocking) plan stream"""
    from abr_control_amd._lib import check, lib

    arr.zero_()
    check(lib().abrk_device_sync(arr.device))


def test_gpu_recorded_plans_equal_direct_calls():
    """Joint / Damping / RestingConfig / Floating / AvoidJointLimits / AvoidObstacles / inverse kinematics / dynamics:
    the recorded plan (launch and hipGraph replay) writes exactly what the direct call writes"""
    import abr_control_amd as a
    from abr_control_amd import engine

    be = cases.GpuBackend("ur5")
    arm, n, B = be.arm_id, 6, 4096
    q, dq, t = draw(71, B, n)
    g = golden("sec_ur5")
    lim = cases.secondary_limit_params(g, "limA", n)
    obs = cases.secondary_obstacle_params(g)
    ikp = _abi.make_ik_params(n_timesteps=20)
    s = a.Stream(0)
    qd, dqd, td = _dev(q, dq, t)
    calls = {
        "joint": lambda u: engine.joint_generate(arm, n, _abi.make_joint(30, 6), True, qd, dqd, td, None, u=u, stream=s),
        "damping": lambda u: engine.joint_generate(arm, n, _abi.make_damping(7), False, qd, dqd, u=u, stream=s),
        "resting": lambda u: engine.joint_generate(arm, n, _abi.make_resting([None, 0.5, 1, None, 2, None], kp=20, kv=4),
                                                   False, qd, dqd, u=u, stream=s),
        "floating": lambda u: engine.floating_generate(arm, n, 1, 1, qd, dqd, u=u, stream=s),
        "limits": lambda u: engine.avoid_joint_limits_generate(n, lim, qd, u=u, stream=s),
        "obstacles": lambda u: engine.avoid_obstacles_generate(arm, n, obs, qd, u=u, stream=s),
    }
    for name, call in calls.items():
        u_direct, u_plan = a.DeviceArray((B, n)), a.DeviceArray((B, n))
        call(u_direct)
        s.sync()
        with engine.Plan(0, s) as plan:
            call(u_plan)
        _zero(u_plan)
        plan.launch()
        s.sync()
        assert np.array_equal(u_plan.numpy(), u_direct.numpy()), name
        _zero(u_plan)
        plan.launch_graph(4)
        s.sync()
        assert np.array_equal(u_plan.numpy(), u_direct.numpy()), name
        assert np.abs(u_direct.numpy()).max() > 0, name
        plan.close()
    # inverse kinematics and the robot_config outputs
    pp, vp = engine.ik_generate_path(arm, n, ikp, qd, td, stream=s)
    pp2, vp2 = a.DeviceArray((B, 20, n)), a.DeviceArray((B, 20, n))
    with engine.Plan(0, s) as plan:
        engine.ik_generate_path(arm, n, ikp, qd, td, stream=s, position_path=pp2, velocity_path=vp2)
        r2 = engine.dynamics(arm, n, qd, dqd, _abi.frame_id("EE", n), None, ("Tx", "J", "M", "g", "C"), np.float64, 0,
                             stream=s)
    plan.launch_graph(2)
    s.sync()
    assert np.array_equal(pp.numpy(), pp2.numpy()) and np.array_equal(vp.numpy(), vp2.numpy())
    r1 = engine.dynamics(arm, n, q, dq, _abi.frame_id("EE", n), None, ("Tx", "J", "M", "g", "C"), np.float64, 0)
    for k in r1:
        assert np.array_equal(r1[k], r2[k].numpy()), k


def test_gpu_recorded_tick_of_three_kernels_equals_the_controller_classes():
    """one plan = AvoidJointLimits -> AvoidObstacles (accumulate) -> OSC with the sum behind its null-space filter
    (osc.py:310-318) == OSC(null_controllers=[limits, obstacles, Damping]).generate of the public classes"""
    import abr_control_amd as a
    from abr_control_amd import engine
    from abr_control_amd.arms import ur5
    from abr_control_amd.controllers import OSC, AvoidJointLimits, AvoidObstacles, Damping

    g = golden("sec_ur5")
    n, B = 6, 2048
    q, dq, t = draw(72, B, n)
    rc = ur5.Config()
    limits = AvoidJointLimits(rc, min_joint_angles=[0.8, None, 1.0, 0.5, None, 2.0],
                              max_joint_angles=[5.0, 4.0, None, 5.5, 3.0, 4.5], max_torque=[30, 20, 10, 5, 5, 2],
                              cross_zero=[False] * 6, gradient=[False, True, False, True, False, False])
    obstacles = AvoidObstacles(rc, obstacles=g["obs_obstacles"], threshold=float(g["obs_threshold"]),
                               gain=float(g["obs_gain"]))
    ctrlr = OSC(rc, kp=100, null_controllers=[limits, obstacles, Damping(rc, kv=10)])
    ref = ctrlr.generate(q, dq, t)
    s = a.Stream(0)
    qd, dqd, td = _dev(q, dq, t)
    une, u = a.DeviceArray((B, n)), a.DeviceArray((B, n))
    params = _abi.make_osc_params(n, kp=100, null_controllers=[_abi.make_damping(10)])
    with engine.Plan(0, s) as tick:
        engine.avoid_joint_limits_generate(n, limits._params, qd, u=une, stream=s)
        engine.avoid_obstacles_generate(rc.arm_id, n, obstacles._params(), qd, u=une, accumulate=True, stream=s)
        engine.osc_generate(rc.arm_id, n, params, qd, dqd, td, u_null_ext=une, u=u, stream=s)
    for launch in (tick.launch, lambda: tick.launch_graph(3)):
        _zero(u)
        launch()
        s.sync()
        assert np.array_equal(u.numpy(), ref)


def test_gpu_plan_slots_are_recycled_and_stale_ids_rejected():
    """re-planning in a loop (gains / targets / buffers change) never exhausts the registry; the payload of a
    destroyed plan is freed, its id stays invalid after the slot has a new tenant"""
    import abr_control_amd as a
    from abr_control_amd import engine
    from abr_control_amd._lib import AbrkError, lib

    be = cases.GpuBackend("ur5")
    q, dq, t = draw(73, 64, 6)
    qd, dqd, td = _dev(q, dq, t)
    u = a.DeviceArray((64, 6))
    s = a.Stream(0)
    base = lib().abrk_plan_count()
    first = engine.OscPlan(be.arm_id, 6, _abi.make_osc_params(6, kp=1.0), qd, dqd, td, u, stream=s)
    stale = first.id
    first.close()
    for i in range(6000):  # more than the 4096 slots
        p = engine.OscPlan(be.arm_id, 6, _abi.make_osc_params(6, kp=float(1 + i)), qd, dqd, td, u, stream=s)
        if i % 1500 == 0:
            p.launch()
        p.close()
    assert lib().abrk_plan_count() == base
    keep = engine.OscPlan(be.arm_id, 6, _abi.make_osc_params(6, kp=5.0), qd, dqd, td, u, stream=s)
    assert (keep.id & 4095) == (stale & 4095) and keep.id != stale  # same slot, new generation
    assert lib().abrk_plan_launch(stale) < 0 and lib().abrk_plan_destroy(stale) < 0
    keep.launch()
    s.sync()
    assert np.array_equal(u.numpy(), be.osc(_abi.make_osc_params(6, kp=5.0), q, dq, t)[0])
    # host pointers cannot be recorded; the failed recording leaves the thread usable
    with pytest.raises(AbrkError):
        with engine.Plan(0, s):
            engine.osc_generate(be.arm_id, 6, _abi.make_osc_params(6), q, dq, t, stream=s)
    assert lib().abrk_plan_count() == base + 1
    with engine.Plan(0, s) as ok:
        engine.osc_generate(be.arm_id, 6, _abi.make_osc_params(6), qd, dqd, td, u=u, stream=s)
    ok.launch()
    s.sync()


def test_gpu_rollout_refuses_unfused_null_controllers_and_gains_are_live():
    """ArmSim.rollout must not silently drop AvoidJointLimits / AvoidObstacles / Floating; the fused
    Damping / RestingConfig gains are read at every generate() (gain scheduling), as the reference does by calling
    null_controller.generate() every tick (osc.py:311-313); more than ABRK_MAX_NULL of them overflow to u_null_ext"""
    from abr_control_amd.arms import twojoint, ur5
    from abr_control_amd.arms.twojoint import ArmSim
    from abr_control_amd.controllers import OSC, AvoidJointLimits, Damping
    from oracle.oracle import Oracle

    rc = twojoint.Config()
    sim = ArmSim(rc, q_init=np.tile(rc.START_ANGLES, (4, 1)))
    lim = AvoidJointLimits(rc, [0.1, 0.1], [3.0, 3.0], [5, 5])
    with pytest.raises(TypeError):
        sim.rollout(OSC(rc, kp=10, ctrlr_dof=cases.XY, null_controllers=[lim]), np.zeros(6), 10)
    with pytest.raises(ValueError):
        sim.rollout(OSC(twojoint.Config(), kp=10, ctrlr_dof=cases.XY), np.zeros(6), 10)
    rc6 = ur5.Config()
    q, dq, t = draw(74, 256, 6)
    damp = Damping(rc6, kv=10)
    c = OSC(rc6, kp=200, null_controllers=[damp])
    o = Oracle(_abi.load_table("ur5"))
    for kv in (10.0, 3.0):
        damp.kv = kv
        ref = o.osc_batch(_abi.make_osc_params(6, kp=200, null_controllers=[_abi.make_damping(kv)]), q, dq, t)
        assert cases.rel_err(c.generate(q, dq, t), ref).max() < 1e-9
    six = [Damping(rc6, kv=k) for k in (1.0, 2.0, 3.0, 4.0, 5.0, 6.0)]  # 4 fused + 2 through u_null_ext
    ref = o.osc_batch(_abi.make_osc_params(6, kp=200, null_controllers=[_abi.make_damping(21.0)]), q, dq, t)
    assert cases.rel_err(OSC(rc6, kp=200, null_controllers=six).generate(q, dq, t), ref).max() < 1e-9


# ---------------------------------------------------------------------------- fused u + Tx, J, M, g (SURVEY 8d Mode F)
@pytest.mark.parametrize("arm,kw", [
    ("ur5", dict(kp=200)),
    ("ur5", dict(kp=200, use_C=True)),
    ("ur5", dict(kp=100, ko=60, kv=12, ctrlr_dof=[1] * 6, use_C=True, ref_frame="link5", xyz_offset=[0.05, 0.0, -0.1],
                 null_controllers=[_abi.make_damping(5)])),
    ("jaco2", dict(kp=200, null_controllers=[_abi.make_damping(10)])),
    ("twojoint", dict(kp=10, kv=3, ctrlr_dof=cases.XY, use_C=True)),
    ("threejoint", dict(kp=50, ctrlr_dof=cases.XY)),
])
@pytest.mark.parametrize("variant", ["static", "rt"])
def test_gpu_fused_full_outputs_equal_separate_calls(arm, kw, variant):
    """abrk_osc_generate_full_batch: u (and training_signal) bit-equal to abrk_osc_generate_batch, and Tx / J / M / g
    equal to abrk_dynamics_batch of the same ref_frame / offset - including the last, partial wavefront and the
    fp32 instantiation"""
    be = cases.GpuBackend(arm, variant)
    n = be.n
    p = _abi.make_osc_params(n, **kw)
    frame, off = kw.get("ref_frame", "EE"), kw.get("xyz_offset")
    for B, dtype, tol in ((1000, np.float64, 1e-13), (77, np.float32, 2e-5)):
        q, dq, t = (x.astype(dtype) for x in draw(81, B, n))
        u0, ts0 = be.e.osc_generate(be.arm_id, n, p, q, dq, t, training_signal=True, dtype=dtype)
        u1, ts1, dyn = be.e.osc_generate(be.arm_id, n, p, q, dq, t, training_signal=True, dtype=dtype,
                                         want=("Tx", "J", "M", "g"))
        ref = be.e.dynamics(be.arm_id, n, q, None, _abi.frame_id(frame, n), off, ("Tx", "J", "M", "g"), dtype, 0)
        scale = lambda x: max(1.0, float(np.max(np.abs(x))))
        # the two kernels schedule the same arithmetic differently (fma contraction): equal to rounding
        assert np.max(np.abs(u1.astype(float) - u0)) <= tol * scale(u0) * 1e3
        assert np.max(np.abs(ts1.astype(float) - ts0)) <= tol * scale(ts0) * 1e3
        for k in ("Tx", "J", "M", "g"):
            assert dyn[k].shape == ref[k].shape and dyn[k].dtype == dtype
            assert np.max(np.abs(dyn[k].astype(float) - ref[k])) <= tol * scale(ref[k]), (arm, variant, k)
        # a subset of outputs leaves the others untouched
        only = be.e.osc_generate(be.arm_id, n, p, q, dq, t, dtype=dtype, want=("M",))[1]
        assert list(only) == ["M"] and np.array_equal(only["M"], dyn["M"])
        # the velocity-dependent robot_config functions too: C(q, dq) and dJ of the same frame / offset
        allw = ("Tx", "J", "M", "g", "C", "dJ")
        u2, ts2, dyn2 = be.e.osc_generate(be.arm_id, n, p, q, dq, t, training_signal=True, dtype=dtype, want=allw)
        ref2 = be.e.dynamics(be.arm_id, n, q, dq, _abi.frame_id(frame, n), off, allw, dtype, 0)
        assert np.max(np.abs(u2.astype(float) - u0)) <= tol * scale(u0) * 1e3
        assert np.max(np.abs(ts2.astype(float) - ts0)) <= tol * scale(ts0) * 1e3
        for k in allw:
            assert dyn2[k].shape == ref2[k].shape and dyn2[k].dtype == dtype
            assert np.max(np.abs(dyn2[k].astype(float) - ref2[k])) <= 10 * tol * scale(ref2[k]), (arm, variant, k)
        cdj = be.e.osc_generate(be.arm_id, n, p, q, dq, t, dtype=dtype, want=("dJ",))[1]
        assert list(cdj) == ["dJ"] and np.array_equal(cdj["dJ"], dyn2["dJ"])


def test_gpu_osc_generate_return_dynamics_python_api():
    from abr_control_amd.arms import ur5
    from abr_control_amd.controllers import OSC

    rc = ur5.Config()
    c = OSC(rc, kp=200, use_C=True)
    q, dq, t = draw(82, 300, 6)
    u, dyn = c.generate(q, dq, t, return_dynamics=("J", "M", "g", "Tx"))
    assert np.allclose(u, c.generate(q, dq, t), rtol=1e-12, atol=1e-12)
    assert np.allclose(dyn["J"], rc.J("EE", q), atol=1e-6) and np.allclose(dyn["M"], rc.M(q), atol=1e-5)
    assert np.allclose(dyn["g"], rc.g(q), atol=1e-5) and np.allclose(dyn["Tx"], rc.Tx("EE", q), atol=1e-12)
    u1, d1 = c.generate(q[0], dq[0], t[0], return_dynamics=("M",))
    assert u1.shape == (6,) and d1["M"].shape == (6, 6)
    # ... and the reference's two most expensive functions from the same launch, against its own outputs
    g = golden("ur5")
    qg, dqg = g["dyn_q"], g["dyn_dq"]
    tg = np.zeros((len(qg), 6))
    _, d2 = c.generate(qg, dqg, tg, return_dynamics=("C", "dJ"))
    assert d2["C"].shape == g["C"].shape and np.max(np.abs(d2["C"] - g["C"])) < 1e-5 * max(1, np.abs(g["C"]).max())
    assert np.max(np.abs(d2["dJ"] - g["dJ_EE"])) < 1e-5 * max(1, np.abs(g["dJ_EE"]).max())


def test_gpu_fp32_runtime_table_sliding_is_as_accurate_as_the_builtin():
    """at 8 M rows the fp32 Sliding result of the threejoint arm on the runtime-table kernels differed
    from the built-in kernels by up to 2.6e-3 relative (profiles/round2/rt_ab.md).  Measured against the fp64 kernels on
    the same float32 inputs (tools/history/gpu_rt_fp32_check.py, profiles/round3/rt_fp32.txt) BOTH fp32 programs are that far
    from fp64 on the same handful of rows - the planar arm folded onto itself (q1 ~ pi, q2 ~ 0), where J[:2] loses rank
    and pinv amplifies rounding - the built-in (6.9e-3) more than the runtime table (4.3e-3).  Pinned here: the
    runtime-table kernels are no further from fp64 than the built-in ones anywhere in the distribution, and wherever the
    built-in result is good to 1e-5 (99.98 % of random states) the two agree to 2e-4."""
    import ctypes as C

    from abr_control_amd import engine
    from abr_control_amd._lib import check, lib

    B = 1 << 22
    tab = _abi.load_table("threejoint")
    p = _abi.make_sliding_params(3)
    rng = np.random.RandomState(1)
    q, dq, t = (rng.uniform(0, 2 * np.pi, (B, 3)).astype(np.float32), rng.uniform(0, 5, (B, 3)).astype(np.float32),
                rng.uniform(-1, 1, (B, 3)).astype(np.float32))
    a_static = check(lib().abrk_arm_builtin(b"threejoint"))
    d = _abi.desc_from_table(tab)
    a_rt = check(lib().abrk_arm_create(C.byref(d)))
    try:
        us = engine.sliding_generate(a_static, 3, p, q, dq, t, dtype=np.float32)
        ur = engine.sliding_generate(a_rt, 3, p, q, dq, t, dtype=np.float32)
    finally:
        lib().abrk_arm_destroy(a_rt)
    u64 = engine.sliding_generate(a_static, 3, p, q.astype(float), dq.astype(float), t.astype(float), dtype=np.float64)
    rel = lambda a, b: np.max(np.abs(a.astype(float) - b), axis=1) / np.max(np.abs(b), axis=1)
    es, er, esr = rel(us, u64), rel(ur, u64), rel(us, ur.astype(float))
    for pct in (50, 99, 99.99):
        assert np.percentile(er, pct) <= 1.5 * np.percentile(es, pct) + 1e-7, pct
    assert np.median(er) < 5e-7 and np.percentile(er, 99) < 5e-6 and np.percentile(er, 99.99) < 5e-5
    assert er.max() <= 4 * es.max() + 1e-4
    good = es <= 1e-5
    assert good.mean() > 0.999 and esr[good].max() < 2e-4 and er[good].max() < 2e-4


# ---------------------------------------------------------------------------- one call over several devices
def test_gpu_sharded_call_equals_unsharded_bitwise():
    """abrk_osc_generate_sharded / sharding.MultiDevice: contiguous row shards, each on its own stream; with one GPU
    every shard maps to device 0 (the multi-GPU placement is the same code with other ordinals).  Bit-equal to the
    single call, for shard counts that do and do not divide the batch, with per-row state and a training signal"""
    from abr_control_amd import engine
    from abr_control_amd.arms import ur5
    from abr_control_amd.controllers import OSC, Damping
    from abr_control_amd.sharding import MultiDevice

    be = cases.GpuBackend("ur5")
    B = 10007
    q, dq, t = draw(91, B, 6)
    tv = np.random.RandomState(92).uniform(-0.5, 0.5, (B, 6))
    p = _abi.make_osc_params(6, kp=100, kv=15, ki=0.2, use_C=True, null_controllers=[_abi.make_damping(5)])
    ie0 = np.zeros((B, 6))
    u0, ts0 = be.e.osc_generate(be.arm_id, 6, p, q, dq, t, tv, ie0, training_signal=True)
    for devices in ([0], [0, 0], [0] * 8, [0] * 13):
        ie = np.zeros((B, 6))
        u, ts = engine.osc_generate_sharded(be.arm_id, 6, p, q, dq, t, devices, tv, ie, training_signal=True)
        assert np.array_equal(u, u0) and np.array_equal(ts, ts0) and np.array_equal(ie, ie0), devices
    # more shards than rows, fp32, and the controller-level API
    u3 = engine.osc_generate_sharded(be.arm_id, 6, _abi.make_osc_params(6, kp=200), q[:3], dq[:3], t[:3], [0] * 8)
    assert np.array_equal(u3, be.e.osc_generate(be.arm_id, 6, _abi.make_osc_params(6, kp=200), q[:3], dq[:3], t[:3]))
    rc = ur5.Config()
    c = OSC(rc, kp=200, null_controllers=[Damping(rc, kv=10)])
    md = MultiDevice([0, 0, 0])
    assert np.array_equal(md.generate(c, q, dq, t), c.generate(q, dq, t))
    assert md.generate(c, q[0], dq[0], t[0]).shape == (6,)
    with pytest.raises(Exception):
        engine.osc_generate_sharded(be.arm_id, 6, p, q, dq, t, [99])


def test_gpu_resident_shards_equal_unsharded_bitwise():
    """SURVEY 8e "results remain in per-device buffers unless the caller asks for host arrays" / VERDICT r5 missing #1:
    shards that LIVE on the devices, one host thread (abrk_*_resident, sharding.ShardedArray + MultiDevice).  With one GPU
    every shard maps to device 0 (devices = [0] * 8: eight shards, eight streams; the multi-GPU placement is the same
    code with other ordinals).  The resident call is `array_equal` to the unsharded one: x,y,z law with Coriolis term,
    fused null controller, target velocity and `ki` state over 5 ticks; the six-row law (hand-over form per shard) with
    and without the training signal; Sliding, Joint, Damping, RestingConfig and the robot_config functions."""
    from abr_control_amd import engine
    from abr_control_amd.arms import ur5
    from abr_control_amd.controllers import OSC, Damping, Joint, RestingConfig, Sliding
    from abr_control_amd.sharding import MultiDevice, ShardedArray

    be = cases.GpuBackend("ur5")
    B = 10007
    q, dq, t = draw(91, B, 6)
    tv = np.random.RandomState(92).uniform(-0.5, 0.5, (B, 6))
    for devices in ([0] * 8, [0, 0, 0], [0] * 13):
        md = MultiDevice(devices)
        qs, dqs, ts_, tvs = (md.scatter(x) for x in (q, dq, t, tv))
        assert np.array_equal(qs.numpy(), q) and qs.rows == ShardedArray.cut(B, len(devices))
        # x,y,z + C + Damping + target velocity + integral state, 5 ticks: the state stays with its shards
        p = _abi.make_osc_params(6, kp=100, kv=15, ki=0.2, use_C=True, null_controllers=[_abi.make_damping(5)])
        ie0, ies = np.zeros((B, 6)), md.zeros((B, 6), np.float64)
        for tick in range(5):
            u0, ts0 = be.e.osc_generate(be.arm_id, 6, p, q, dq, t, tv, ie0, training_signal=True)
            u, tsg = engine.osc_generate_resident(be.arm_id, 6, p, qs, dqs, ts_, tvs, ies, training_signal=True,
                                                  streams=md.streams)
            md.sync()
            assert np.array_equal(u.numpy(), u0) and np.array_equal(tsg.numpy(), ts0), (devices, tick)
            assert np.array_equal(ies.numpy(), ie0), (devices, tick)
        # six task rows: every shard runs first pass + finish kernel on its own (device, stream) scratch
        p6 = _abi.make_osc_params(6, kp=200, ko=150, kv=25, ctrlr_dof=[1] * 6)
        u6 = be.e.osc_generate(be.arm_id, 6, p6, q, dq, t)
        assert np.array_equal(engine.osc_generate_resident(be.arm_id, 6, p6, qs, dqs, ts_).numpy(), u6), devices
        u6t, ts6 = be.e.osc_generate(be.arm_id, 6, p6, q, dq, t, training_signal=True)
        r = engine.osc_generate_resident(be.arm_id, 6, p6, qs, dqs, ts_, training_signal=True)
        assert np.array_equal(r[0].numpy(), u6t) and np.array_equal(r[1].numpy(), ts6), devices
    # the controller classes over ShardedArrays: MultiDevice.generate only enqueues, .numpy() gathers
    md = MultiDevice([0] * 8)
    qs, dqs, ts_ = (md.scatter(x) for x in (q, dq, t))
    rc = ur5.Config()
    c = OSC(rc, kp=200, ki=0.1, null_controllers=[Damping(rc, kv=10)])
    c_ref = OSC(rc, kp=200, ki=0.1, null_controllers=[Damping(rc, kv=10)])
    for tick in range(3):
        us = md.generate(c, qs, dqs, ts_)
        assert isinstance(us, ShardedArray)
        assert np.array_equal(us.numpy(), c_ref.generate(q, dq, t)), tick
    assert np.array_equal(c.integrated_error.numpy(), c_ref.integrated_error)
    assert np.array_equal(c.training_signal.numpy(), c_ref.training_signal)
    sl = Sliding(rc)
    t3 = md.scatter(t[:, :3])
    assert np.array_equal(md.generate(sl, qs, dqs, t3).numpy(), Sliding(rc).generate(q, dq, t[:, :3]))
    tj = md.scatter(t)
    assert np.array_equal(md.generate(Joint(rc, kp=20, kv=4), qs, dqs, tj).numpy(), Joint(rc, kp=20, kv=4).generate(q, dq, t))
    assert np.array_equal(md.generate(Damping(rc, kv=7), qs, dqs).numpy(), Damping(rc, kv=7).generate(q, dq))
    rest = [None, 0.8, -1.6, None, 1.5, None]
    assert np.array_equal(md.generate(RestingConfig(rc, rest, kp=30, kv=6), qs, dqs).numpy(),
                          RestingConfig(rc, rest, kp=30, kv=6).generate(q, dq))
    want = ("Tx", "J", "M", "g", "C", "dJ", "quat")
    rr = engine.dynamics_resident(be.arm_id, 6, qs, dqs, want=want)
    ref = be.e.dynamics(be.arm_id, 6, q, dq, None, None, want, np.float64, 0)
    for k in want:
        assert np.array_equal(rr[k].numpy(), ref[k]), k
    # fp32, fewer rows than shards (empty shards are skipped), errors
    p = _abi.make_osc_params(6, kp=200)
    md3 = MultiDevice([0] * 8)
    q3, dq3, t3_ = (md3.scatter(x[:3].astype(np.float32)) for x in (q, dq, t))
    u3 = engine.osc_generate_resident(be.arm_id, 6, p, q3, dq3, t3_, dtype=np.float32)
    assert np.array_equal(u3.numpy(), be.e.osc_generate(be.arm_id, 6, p, q[:3].astype(np.float32), dq[:3].astype(np.float32),
                                                       t[:3].astype(np.float32), dtype=np.float32))
    with pytest.raises(ValueError):
        engine.osc_generate_resident(be.arm_id, 6, p, qs, dq3, ts_)  # cut differently
    with pytest.raises(Exception, match="host arrays|NumPy"):
        engine.osc_generate_sharded(be.arm_id, 6, p, qs.parts[0], dq, t, [0])


def test_gpu_resident_sharded_plan_replays_k_ticks_on_every_shard():
    """a recorded Plan per shard, replayed from ONE call (MultiDevice.record_generate -> ShardedPlan.launch /
    .launch_graph -> abrk_plans_launch): K ticks of a control loop with integral state on eight shards equal K consecutive
    unsharded calls, plain launches and hipGraph replays alike; a singular shard is reported by ShardedPlan.sync()"""
    from abr_control_amd import engine
    from abr_control_amd.arms import ur5
    from abr_control_amd.controllers import OSC, Damping
    from abr_control_amd.sharding import MultiDevice

    B, K = 40000, 6
    q, dq, t = draw(93, B, 6)
    rc = ur5.Config()
    mk = lambda: OSC(rc, kp=100, kv=15, ki=0.2, use_C=True, null_controllers=[Damping(rc, kv=5)])
    ref = mk()
    for _ in range(2 * K):
        u_ref = ref.generate(q, dq, t)
    md = MultiDevice([0] * 8)
    qs, dqs, ts_ = (md.scatter(x) for x in (q, dq, t))
    c = mk()
    plan = md.record_generate(c, qs, dqs, ts_)
    plan.launch(K)          # K plain launches per shard, one call
    plan.launch_graph(K)    # K more ticks as one hipGraph per shard, one call
    plan.sync()
    assert np.array_equal(plan.u.numpy(), u_ref)
    assert np.array_equal(c.integrated_error.numpy(), ref.integrated_error)
    # the six-row law as a sharded plan (every shard's plan owns its worklist / records)
    c6, r6 = OSC(rc, kp=200, ko=150, kv=25, ctrlr_dof=[True] * 6), OSC(rc, kp=200, ko=150, kv=25, ctrlr_dof=[True] * 6)
    plan6 = md.record_generate(c6, qs, dqs, ts_)
    plan6.launch_graph(3)
    plan6.sync()
    assert np.array_equal(plan6.u.numpy(), r6.generate(q, dq, t))
    assert np.array_equal(c6.training_signal.numpy(), r6.training_signal)
    # ... and without the training signal: the NOTS kernels, bit-equal to the unsharded call that asks for none either
    plan6n = md.record_generate(c6, qs, dqs, ts_, training_signal=False)
    plan6n.launch(2)
    plan6n.sync()
    assert np.array_equal(plan6n.u.numpy(), engine.osc_generate(rc.arm_id, 6, c6._params("EE", None), q, dq, t))
    plan6n.close()
    plan.close()
    plan6.close()
    # new states into the fixed buffers between ticks
    q2, dq2, t2 = draw(94, B, 6)
    qs.copy_from_numpy(q2), dqs.copy_from_numpy(dq2), ts_.copy_from_numpy(t2)
    c2 = OSC(rc, kp=200)
    plan2 = md.record_generate(c2, qs, dqs, ts_)
    plan2.launch()
    plan2.sync()
    assert np.array_equal(plan2.u.numpy(), OSC(rc, kp=200).generate(q2, dq2, t2))
    plan2.close()


def test_gpu_resident_shards_from_threads_and_host_sharded_calls_on_disjoint_slots():
    """the host-array *_sharded calls no longer serialise on a process-wide lock (one lock per device, one host thread per
    device inside a call) and resident calls take none: four threads mixing both on one device return the single-call
    bits (TSan run: tools/gpu_sanitize.sh)"""
    import threading

    from abr_control_amd import engine
    from abr_control_amd.sharding import MultiDevice

    be = cases.GpuBackend("ur5")
    p = _abi.make_osc_params(6, kp=200, use_C=True)
    p6 = _abi.make_osc_params(6, kp=200, ko=150, kv=25, ctrlr_dof=[1] * 6)
    data = [draw(100 + i, 6000 + 37 * i, 6) for i in range(4)]
    want = [(be.e.osc_generate(be.arm_id, 6, p, *d), be.e.osc_generate(be.arm_id, 6, p6, *d)) for d in data]
    bad = []

    def work(i):
        try:
            q, dq, t = data[i]
            for rep in range(6):
                if (i + rep) % 2:
                    u = engine.osc_generate_sharded(be.arm_id, 6, p, q, dq, t, [0] * (2 + i))
                    u6 = engine.osc_generate_sharded(be.arm_id, 6, p6, q, dq, t, [0] * (2 + i))
                else:
                    import abr_control_amd as a

                    md = MultiDevice([0] * (2 + i))
                    own = [a.Stream(0) for _ in md.devices]  # this thread's own streams: nothing shared with the others
                    qs, dqs, ts_ = (md.scatter(x) for x in (q, dq, t))
                    ud = engine.osc_generate_resident(be.arm_id, 6, p, qs, dqs, ts_, streams=own)
                    u6d = engine.osc_generate_resident(be.arm_id, 6, p6, qs, dqs, ts_, streams=own)
                    engine.shards_sync(ud, own)
                    u, u6 = ud.numpy(own), u6d.numpy(own)
                if not (np.array_equal(u, want[i][0]) and np.array_equal(u6, want[i][1])):
                    bad.append((i, rep))
        except Exception as e:  # noqa: BLE001
            bad.append((i, repr(e)))

    ths = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not bad, bad


def test_gpu_sharded_sliding_joint_dynamics_equal_unsharded_bitwise():
    """VERDICT r2 #5d: the one-call-every-device path for the other entry points of the hot path - Sliding (BASELINE
    config 5), Joint / Damping / RestingConfig and the robot_config functions - through the C ABI
    (abrk_*_sharded) and through sharding.MultiDevice; shards mapped onto device 0, bit-equal to the single call"""
    from abr_control_amd import engine
    from abr_control_amd.arms import threejoint, ur5
    from abr_control_amd.controllers import Damping, Joint, RestingConfig, Sliding
    from abr_control_amd.sharding import MultiDevice

    # Sliding, fp32, BASELINE config 5's arm; batch sizes the shard counts do and do not divide
    be3 = cases.GpuBackend("threejoint")
    B = 65536 + 5
    q, dq, _ = draw(93, B, 3)
    t = np.random.RandomState(94).uniform(-1, 1, (B, 3))
    tv = np.random.RandomState(95).uniform(-0.2, 0.2, (B, 3))
    ps = _abi.make_sliding_params(3)
    for dtype in (np.float32, np.float64):
        a = [x.astype(dtype) for x in (q, dq, t, tv)]
        u0, s0 = engine.sliding_generate(be3.arm_id, 3, ps, a[0], a[1], a[2], a[3], want_s=True, dtype=dtype)
        for devices in ([0], [0, 0], [0] * 7):
            u, s = engine.sliding_generate_sharded(be3.arm_id, 3, ps, a[0], a[1], a[2], devices, a[3], want_s=True, dtype=dtype)
            assert np.array_equal(u, u0) and np.array_equal(s, s0), (dtype, devices)
    md = MultiDevice([0, 0, 0])
    rc3 = threejoint.Config()
    sl = Sliding(rc3)
    u_md = md.generate(sl, q, dq, t, tv)
    s_md = sl.s
    assert np.array_equal(u_md, sl.generate(q, dq, t, tv)) and np.array_equal(s_md, sl.s) and not hasattr(sl, "_shard_devices")
    assert md.generate(sl, q[0], dq[0], t[0]).shape == (3,)
    # Joint family on the UR5
    be = cases.GpuBackend("ur5")
    B = 20011
    q, dq, _ = draw(96, B, 6)
    tj = np.random.RandomState(97).uniform(0, 2 * np.pi, (B, 6))
    rc = ur5.Config()
    for c, args in ((Joint(rc, kp=50, kv=7), (tj,)), (Damping(rc, kv=10), ()),
                    (RestingConfig(rc, [None, 1.0, 2.0, None, 0.5, None], kp=30), ())):
        assert np.array_equal(md.generate(c, q, dq, *args), c.generate(q, dq, *args)), type(c).__name__
    u0 = engine.joint_generate(be.arm_id, 6, _abi.make_joint(50, 7), True, q, dq, tj)
    assert np.array_equal(engine.joint_generate_sharded(be.arm_id, 6, _abi.make_joint(50, 7), True, q, dq, [0] * 5, tj), u0)
    # robot_config functions: every output of one launch, incl. the velocity-dependent ones
    want = ("Tx", "J", "M", "g", "C", "dJ", "R", "T", "Tinv", "quat")
    d0 = engine.dynamics(be.arm_id, 6, q, dq, _abi.frame_id("link4", 6), [0.1, -0.05, 0.2], want)
    d1 = engine.dynamics_sharded(be.arm_id, 6, q, [0, 0, 0, 0], dq, _abi.frame_id("link4", 6), [0.1, -0.05, 0.2], want)
    for k in want:
        assert np.array_equal(d0[k], d1[k]), k
    d2 = md.dynamics(rc, q, dq, "link4", [0.1, -0.05, 0.2], want)
    assert all(np.array_equal(d0[k], d2[k]) for k in want)
    assert md.dynamics(rc, q[0])["M"].shape == (6, 6)
    with pytest.raises(Exception):
        engine.sliding_generate_sharded(be3.arm_id, 3, ps, q[:, :3], dq[:, :3], t, [99])
    with pytest.raises(Exception):
        engine.dynamics_sharded(be.arm_id, 6, q, [0], None, None, None, ("C",))  # C needs dq


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gpu_batch_sharded_and_resident_forms_agree_for_every_set_of_optional_arrays(dtype):
    """The three forms of the four sharded families read one table of the family's arrays: `*_batch` on host arrays,
    `*_sharded` and `*_resident` are `array_equal` for every set of optional arrays, i.e. wherever an array is absent
    in the middle of the list.  UR5, 131 rows over devices [0, 0, 0]: shards of 44, 44 and 43 rows, none a whole
    wavefront.  OSC runs two ticks each, so that the in/out integral state is compared too."""
    from itertools import product

    from abr_control_amd import engine
    from abr_control_amd.sharding import MultiDevice

    arm, B, devices = cases.GpuBackend("ur5").arm_id, 131, [0, 0, 0]
    md = MultiDevice(devices)
    rs = np.random.RandomState(133)
    q, dq, t = (x.astype(dtype) for x in draw(131, B, 6))
    tv, une, ta = (rs.uniform(-0.5, 0.5, (B, 6)).astype(dtype) for _ in range(3))
    qs, dqs, ts_, tvs, unes, tas = (md.scatter(x) for x in (q, dq, t, tv, une, ta))
    assert qs.rows == [44, 44, 43]

    def same(batch, sharded, resident, what):
        for b, s, r in zip(*((x if isinstance(x, tuple) else (x,)) for x in (batch, sharded, resident))):
            assert np.array_equal(s, b) and np.array_equal(r.numpy(), b), what

    def osc(dof, with_tv, with_ie, with_une, with_ts):
        what = (dof, with_tv, with_ie, with_une, with_ts)
        p = _abi.make_osc_params(6, kp=100, ko=80, kv=15, ki=0.2 if with_ie else 0, ctrlr_dof=dof)
        ie_b, ie_s = (np.zeros((B, 6), dtype) if with_ie else None for _ in range(2))
        ie_r = md.scatter(np.zeros((B, 6), dtype)) if with_ie else None
        pick = lambda use, x: x if use else None
        for tick in range(2):
            kw = dict(training_signal=with_ts, dtype=dtype)
            same(engine.osc_generate(arm, 6, p, q, dq, t, pick(with_tv, tv), ie_b, pick(with_une, une), **kw),
                 engine.osc_generate_sharded(arm, 6, p, q, dq, t, devices, pick(with_tv, tv), ie_s, pick(with_une, une), **kw),
                 engine.osc_generate_resident(arm, 6, p, qs, dqs, ts_, pick(with_tv, tvs), ie_r, pick(with_une, unes), **kw),
                 what + (tick,))
            if with_ie:
                assert ie_b.any() and np.array_equal(ie_s, ie_b) and np.array_equal(ie_r.numpy(), ie_b), what + (tick,)

    for subset in product((False, True), repeat=4):
        osc([1, 1, 1, 0, 0, 0], *subset)
    osc([1] * 6, True, True, True, True)

    ps = _abi.make_sliding_params(6)
    for with_tv, with_ta, with_s in product((False, True), repeat=3):
        pick = lambda use, x: x[:, :3] if use else None
        tv3, ta3, tvs3, tas3 = pick(with_tv, tv), pick(with_ta, ta), None, None
        if with_tv:
            tvs3 = md.scatter(tv3)
        if with_ta:
            tas3 = md.scatter(ta3)
        same(engine.sliding_generate(arm, 6, ps, q, dq, t[:, :3], tv3, ta3, want_s=with_s, dtype=dtype),
             engine.sliding_generate_sharded(arm, 6, ps, q, dq, t[:, :3], devices, tv3, ta3, want_s=with_s, dtype=dtype),
             engine.sliding_generate_resident(arm, 6, ps, qs, dqs, md.scatter(t[:, :3]), tvs3, tas3, want_s=with_s,
                                              dtype=dtype),
             ("sliding", with_tv, with_ta, with_s))

    for ctrl, target, velocity in ((_abi.make_joint(50, 7), True, True), (_abi.make_joint(50, 7), True, False),
                                   (_abi.make_damping(10), False, False)):
        pick = lambda use, x: x if use else None
        same(engine.joint_generate(arm, 6, ctrl, True, q, dq, pick(target, t), pick(velocity, tv), dtype=dtype),
             engine.joint_generate_sharded(arm, 6, ctrl, True, q, dq, devices, pick(target, t), pick(velocity, tv),
                                           dtype=dtype),
             engine.joint_generate_resident(arm, 6, ctrl, True, qs, dqs, pick(target, ts_), pick(velocity, tvs),
                                            dtype=dtype),
             ("joint", ctrl.kind, target, velocity))

    frame, x_off = _abi.frame_id("link4", 6), [0.1, -0.05, 0.2]
    every = ("Tx", "J", "M", "g", "C", "dJ", "R", "T", "Tinv", "quat")
    for want, with_dq in ((every, True), (("M",), False), (("Tx", "dJ", "quat"), True)):
        b = engine.dynamics(arm, 6, q, dq if with_dq else None, frame, x_off, want, dtype)
        s = engine.dynamics_sharded(arm, 6, q, devices, dq if with_dq else None, frame, x_off, want, dtype)
        r = engine.dynamics_resident(arm, 6, qs, dqs if with_dq else None, frame, x_off, want, dtype)
        assert set(b) == set(s) == set(r) == set(want)
        for k in want:
            assert np.array_equal(s[k], b[k]) and np.array_equal(r[k].numpy(), b[k]), (want, k)


# ---------------------------------------------------------------------------- the wave-cooperative mapping (north_star)
@pytest.mark.parametrize("lanes", [4, 8, 16])
def test_gpu_wave_cooperative_variant_matches_reference_and_lane_per_arm(lanes):
    """K lanes per arm, frames / Jacobian columns / M staged in LDS (abrk_coop.h): same results as the reference
    (golden cfg2, incl. its truncated-pinv rows) and as the lane-per-arm kernel, for batches that do not fill the
    last wavefront; vmax and use_g honoured; unsupported options refused"""
    from abr_control_amd import engine
    from abr_control_amd._lib import AbrkError

    be = cases.GpuBackend("ur5")
    g = golden("ur5")
    q, dq, t = g["cfg2_q"], g["cfg2_dq"], g["cfg2_target"]
    p = _abi.make_osc_params(6, kp=200)
    u, ts = engine.osc_generate_coop(be.arm_id, 6, p, q, dq, t, lanes, training_signal=True)
    ok = ~cases.threshold_band(g, "cfg2")
    assert cases.rel_err(u, g["cfg2_uD"])[ok].max() <= cases.TOL_D
    assert cases.rel_err(ts, g["cfg2_tsD"])[ok].max() <= cases.TOL_D
    for B, kw in ((1, dict(kp=200)), (67, dict(kp=30, kv=7, use_g=False)), (1003, dict(kp=100, kv=15, vmax=[0.5, 1.0]))):
        qq, dd, tt = draw(95 + B, B, 6)
        pp = _abi.make_osc_params(6, **kw)
        ref = be.osc(pp, qq, dd, tt)[0]
        got = engine.osc_generate_coop(be.arm_id, 6, pp, qq, dd, tt, lanes)
        assert cases.rel_err(got, ref).max() <= 1e-9, (B, kw)
    for bad in (dict(use_C=True), dict(ctrlr_dof=[1] * 6), dict(null_controllers=[_abi.make_damping(5)]), dict(ki=0.1),
                dict(xyz_offset=[0.1, 0, 0])):
        with pytest.raises(AbrkError):
            engine.osc_generate_coop(be.arm_id, 6, _abi.make_osc_params(6, **bad), q[:4], dq[:4], t[:4], lanes)
    with pytest.raises(AbrkError):
        engine.osc_generate_coop(cases.GpuBackend("jaco2").arm_id, 6, p, q[:4], dq[:4], t[:4], lanes)


# ---------------------------------------------------------------------------- six-row law: Jacobi rows deferred to a dense pass
@pytest.mark.parametrize("variant", ["static", "rt"])
def test_gpu_six_row_deferred_pass_equals_inline_sweeps(variant):
    """With all six task rows most wavefronts hold a row whose pinv truncates; those rows are parked in a worklist and
    worked off by a second, densely packed pass (abrk_kernels.h osc_kernel modes 1 / 2).  Batches below 16384 rows run
    the sweeps inline: chunked calls must reproduce the one big call bit for bit - u, training signal and the per-row
    integral state - directly, through a recorded plan, and replayed as a hipGraph"""
    import abr_control_amd as a
    from abr_control_amd import engine

    be = cases.GpuBackend("ur5", variant)
    B = 40000
    q, dq, t = draw(97, B, 6)
    for kw in (dict(kp=200, ko=150, kv=25, ctrlr_dof=[1] * 6),
               dict(kp=100, ko=60, kv=12, ki=0.2, ctrlr_dof=[1, 0, 1, 1, 1, 0], orientation_algorithm=1, use_C=True,
                    null_controllers=[_abi.make_damping(5)])):
        p = _abi.make_osc_params(6, **kw)
        stateful = bool(kw.get("ki"))
        ie_big = np.zeros((B, 6)) if stateful else None
        u_big, ts_big = be.e.osc_generate(be.arm_id, 6, p, q, dq, t, integrated_error=ie_big, training_signal=True)
        u_c, ts_c, ie_c = np.empty_like(u_big), np.empty_like(ts_big), np.zeros((B, 6))
        for lo in range(0, B, 8000):
            sl = slice(lo, lo + 8000)
            ie = np.zeros((len(q[sl]), 6)) if stateful else None
            u_c[sl], ts_c[sl] = be.e.osc_generate(be.arm_id, 6, p, q[sl], dq[sl], t[sl], integrated_error=ie,
                                                  training_signal=True)
            if stateful:
                ie_c[sl] = ie
        assert np.array_equal(u_big, u_c) and np.array_equal(ts_big, ts_c)
        if stateful:
            assert np.array_equal(ie_big, ie_c)
        # the truncating rows really are there (otherwise this test would not exercise the second pass)
        from oracle.oracle import Oracle

        uo = Oracle(_abi.load_table("ur5")).osc_batch(p, q[:600], dq[:600], t[:600], None,
                                                      np.zeros((600, 6)) if stateful else None, None)
        assert np.median(cases.rel_err(u_big[:600], uo)) < 1e-9
        # recorded plan + graph replay on device arrays (stateless case: replaying twice must not change u)
        if not stateful:
            s = a.Stream(0)
            qd, dqd, td = _dev(q, dq, t)
            u = a.DeviceArray((B, 6))
            with engine.Plan(0, s) as plan:
                engine.osc_generate(be.arm_id, 6, p, qd, dqd, td, u=u, stream=s)
            _zero(u)
            plan.launch()
            s.sync()
            # no training signal asked for: the first pass is the NOTS instantiation (gravity joins the velocity term
            # before the factorisations) - the same u to rounding, not to the bit
            u_plan = u.numpy()
            assert np.max(np.abs(u_plan - u_big) / np.max(np.abs(u_big), axis=1, keepdims=True)) < 1e-13
            _zero(u)
            plan.launch_graph(3)
            s.sync()
            assert np.array_equal(u.numpy(), u_plan)
            plan.close()
    # the fp32 instantiation takes the same two passes
    p = _abi.make_osc_params(6, kp=200, ko=150, kv=25, ctrlr_dof=[1] * 6)
    q32, dq32, t32 = (x.astype(np.float32) for x in (q, dq, t))
    big = be.e.osc_generate(be.arm_id, 6, p, q32, dq32, t32, dtype=np.float32)
    chunks = [be.e.osc_generate(be.arm_id, 6, p, q32[lo:lo + 8000], dq32[lo:lo + 8000], t32[lo:lo + 8000], dtype=np.float32)
              for lo in range(0, B, 8000)]
    chunks = np.concatenate(chunks)
    assert big.dtype == np.float32 and np.array_equal(np.isnan(big), np.isnan(chunks))
    # (no training signal: NOTS first pass against the inline program of the chunks - equal to fp32 rounding; the rows
    #  the second pass works off run the very same program in both and are bit-equal)
    fin = np.isfinite(big).all(axis=1)
    rel = np.max(np.abs(big[fin].astype(float) - chunks[fin]), axis=1) / np.max(np.abs(chunks[fin]), axis=1)
    assert np.median(rel) < 1e-6 and np.percentile(rel, 99) < 1e-4
    big_ts = be.e.osc_generate(be.arm_id, 6, p, q32, dq32, t32, training_signal=True, dtype=np.float32)[0]
    chunks_ts = np.concatenate([be.e.osc_generate(be.arm_id, 6, p, q32[lo:lo + 8000], dq32[lo:lo + 8000], t32[lo:lo + 8000],
                                                  training_signal=True, dtype=np.float32)[0] for lo in range(0, B, 8000)])
    assert np.array_equal(big_ts, chunks_ts, equal_nan=True)  # with it: the same arithmetic, bit for bit


@pytest.mark.parametrize("arm,variant", [("ur5", "static"), ("ur5", "rt"), ("jaco2", "static")])
def test_gpu_six_row_handover_near_singular_postures(arm, variant):
    """batches of 64 to 65 536 rows run the six-row law as first pass + finish kernel on hand-over records (a deferring
    row leaves Mx_inv, its task Jacobian rows, u_task and the joint-space sums; osc6_finish_kernel - one deferred row
    per wavefront, each lane one column - completes it; 600 rows here: the per-chunk kernel): hundreds of truncating rows (postures next to the kinematic
    singularities), plain law / Coriolis + two fused secondary controllers / target velocity + integral state over two
    steps + external null-space signal, against the oracle"""
    be = cases.GpuBackend(arm, variant)
    worst, n_trunc = cases.check_six_row_near_singular(be, arm, B=600)
    assert n_trunc > 120 and worst <= cases.TOL_D


_FORMS_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from abr_control_amd import _abi
from tests import cases
d = np.load(sys.argv[2])
be = cases.GpuBackend(str(d["arm"]))
out = {}
for i, kw in enumerate((dict(kp=200, ko=150, kv=25, ctrlr_dof=[1] * 6),
                        dict(kp=100, ko=60, kv=12, ctrlr_dof=[1, 0, 1, 1, 1, 0], orientation_algorithm=1, use_C=True,
                             null_controllers=[_abi.make_damping(5)]))):
    for dt in (np.float64, np.float32):
        u, ts = be.osc(_abi.make_osc_params(6, **kw), d["q"].astype(dt), d["dq"].astype(dt), d["t"].astype(dt), dtype=dt)
        out[f"u{i}_{np.dtype(dt).name}"], out[f"ts{i}_{np.dtype(dt).name}"] = u, ts
np.savez(sys.argv[3], **out)
"""


def test_gpu_six_row_finish_forms_agree_bitwise(tmp_path):
    """the finish kernel takes one record per WAVEFRONT (chunks with few of them) or one per LANE (many): a row's result
    must not depend on which ran - the two are different instantiations of the same solver with contraction pinned off.
    The same batch forced through each form (measurement switches ABRK_FINISH_ROUNDS / _SLOTS: no cooperative round at
    all; 4 wavefronts per chunk that take up to 16 records each, one after the other), fp64 and fp32, a batch that ends
    in a partial chunk, a controller whose every row truncates (64 records per chunk): equal bit for bit, and equal to
    what the default rule picks"""
    import subprocess
    import sys

    from tests.conftest import REPO

    qs = cases.near_singular_postures("ur5", 600)
    rng = np.random.RandomState(5)
    q = np.concatenate([qs, rng.uniform(0, 2 * np.pi, (3000 - len(qs), 6))])
    dq, t = rng.uniform(0, 5, (len(q), 6)), rng.uniform(-1, 1, (len(q), 6))
    np.savez(tmp_path / "in.npz", arm="ur5", q=q, dq=dq, t=t)
    (tmp_path / "run.py").write_text(_FORMS_SCRIPT)
    res = {}
    # (the switches are read only under ABRK_MEASUREMENT=1: csrc/abrk_kernels.h measurement_env)
    forms = (("lane", dict(ABRK_MEASUREMENT="1", ABRK_FINISH_ROUNDS="0")),
             ("wave", dict(ABRK_MEASUREMENT="1", ABRK_FINISH_ROUNDS="64", ABRK_FINISH_SLOTS="4")),
             ("onepass", dict(ABRK_MEASUREMENT="1", ABRK_NO_DEFER="1")),  # the complete row program, no second pass at all
             # the grouped finish kernel (the 16384-row band's default): 16 and 3 chunks per group
             ("group16", dict(ABRK_MEASUREMENT="1", ABRK_FINISH_GROUP="16")),
             ("group3", dict(ABRK_MEASUREMENT="1", ABRK_FINISH_GROUP="3", ABRK_FINISH_ROUNDS="64")),
             ("default", {}))
    for name, sw in forms:
        env = {k: v for k, v in os.environ.items() if not k.startswith(("ABRK_FINISH_", "ABRK_MEASUREMENT", "ABRK_NO_"))}  # noqa: E501
        env.update(sw)
        r = subprocess.run([sys.executable, str(tmp_path / "run.py"), REPO, str(tmp_path / "in.npz"),
                            str(tmp_path / f"{name}.npz")], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        res[name] = np.load(tmp_path / f"{name}.npz")
    for k in res["lane"].files:
        assert np.array_equal(res["lane"][k], res["wave"][k], equal_nan=True), k
        assert np.array_equal(res["lane"][k], res["default"][k], equal_nan=True), k
        # round 5: the complete row program hands its truncating rows to the same routine the finish kernel runs
        assert np.array_equal(res["lane"][k], res["onepass"][k], equal_nan=True), k
        assert np.array_equal(res["lane"][k], res["group16"][k], equal_nan=True), k
        assert np.array_equal(res["lane"][k], res["group3"][k], equal_nan=True), k
    # ... and the truncating rows are there and right
    uo, _ = cases.OracleBackend("ur5").osc(_abi.make_osc_params(6, kp=200, ko=150, kv=25, ctrlr_dof=[1] * 6), q[600:1100],
                                           dq[600:1100], t[600:1100])
    assert np.median(cases.rel_err(res["wave"]["u0_float64"][600:1100], uo)) < 1e-10


def test_gpu_six_row_many_short_lived_streams():
    """the six-row kernels keep their worklist and hand-over records per (device, stream): a stream that is destroyed
    through the library hands its slot back (device memory stays flat over 200 create - use - destroy cycles), streams
    that stay alive beyond the cache's 64 slots recycle the least recently used idle slot, and no call ever falls back
    to the one-pass form for want of scratch"""
    import abr_control_amd as a
    from abr_control_amd import engine

    be = cases.GpuBackend("ur5")
    p = _abi.make_osc_params(6, kp=200, ko=150, kv=25, ctrlr_dof=[1] * 6)
    B = 2048
    q, dq, t = draw(11, B, 6)
    qd, dqd, td = _dev(q, dq, t)
    u0 = a.DeviceArray((B, 6))
    engine.osc_generate(be.arm_id, 6, p, qd, dqd, td, u=u0)  # (no training signal asked for: the same first pass as below)
    ref = u0.numpy()
    uo, _ = cases.OracleBackend("ur5").osc(p, q[:256], dq[:256], t[:256])
    assert np.median(cases.rel_err(ref[:256], uo)) < 1e-10
    base = a.scratch_stats(0)
    free = []
    for i in range(200):
        s = a.Stream(0)
        u = a.DeviceArray((B, 6))
        engine.osc_generate(be.arm_id, 6, p, qd, dqd, td, u=u, stream=s)
        s.sync()
        if i % 20 == 0:
            assert np.array_equal(u.numpy(), ref)
        del s, u
        if i >= 4:
            free.append(a.scratch_stats(0)["device_free_bytes"])
    st = a.scratch_stats(0)
    assert st["inline_fallbacks"] == base["inline_fallbacks"]
    assert st["worklist_slots"] <= base["worklist_slots"] + 1
    assert max(free) - min(free) <= 64 << 20, (min(free), max(free))
    # 80 streams alive at once: more than the cache holds - the idle ones make room, nothing runs one-pass
    keep = [a.Stream(0) for _ in range(80)]
    outs = []
    for s in keep:
        u = a.DeviceArray((B, 6))
        engine.osc_generate(be.arm_id, 6, p, qd, dqd, td, u=u, stream=s)
        s.sync()  # (an idle stream's slot may be recycled; one with work in flight is never touched)
        outs.append(u)
    for u in outs:
        assert np.array_equal(u.numpy(), ref)
    st2 = a.scratch_stats(0)
    assert st2["inline_fallbacks"] == base["inline_fallbacks"]
    assert st2["evictions"] > st["evictions"] and st2["worklist_slots"] <= 64
    del keep, outs
    assert a.scratch_stats(0)["worklist_slots"] <= base["worklist_slots"] + 1


def test_gpu_six_row_bits_do_not_depend_on_the_batch_size():
    """The six-row law runs one-pass below 64 rows, as first pass + per-chunk or grouped finish kernel on hand-over
    records up to 65536 rows, as first pass + dense finish kernel on hand-over records up to 1 M rows, and as first pass +
    recompute pass beyond (that form and the 0.26 - 1 M row band: tests/test_gpu_six_row_large_batches.py).  Since round
    5 every form hands a truncating row to ONE routine (csrc/abrk_ctrl.h osc6_tail) and runs the same arithmetic around
    it (with and without a training signal among the outputs): a batch just above the 65536-row threshold (dense finish
    form), its halves, 50-row slices of it (one-pass) and an uneven sharded call return the same bits on every row - and
    meet the oracle on a sample."""
    from abr_control_amd import engine

    be = cases.GpuBackend("ur5")
    B = 65536 + 128
    q, dq, t = draw(77, B, 6)
    # near-singular postures among the first rows: truncating rows in every slice below
    qs = cases.near_singular_postures("ur5", 200)
    q[:len(qs)] = qs
    h = B // 2
    for kw in (dict(kp=200, ko=150, kv=25, ctrlr_dof=[1] * 6),
               dict(kp=100, ko=60, kv=12, ctrlr_dof=[1, 1, 1, 1, 1, 0], use_C=True,
                    null_controllers=[_abi.make_damping(5)])):
        p = _abi.make_osc_params(6, **kw)
        u_big, ts_big = be.osc(p, q, dq, t)                                    # dense finish form
        u_a, ts_a = be.osc(p, q[:h], dq[:h], t[:h])                            # hand-over form
        u_b, ts_b = be.osc(p, q[h:], dq[h:], t[h:])
        assert np.all(np.isfinite(u_big))
        assert np.array_equal(u_big, np.concatenate([u_a, u_b])) and np.array_equal(ts_big, np.concatenate([ts_a, ts_b]))
        # 16384 rows: the grouped finish kernel (16 chunks share 64 wavefronts); 12000 rows: a partial last group
        for nb in (16384, 12000):
            u_g, ts_g = be.osc(p, q[:nb], dq[:nb], t[:nb])
            assert np.array_equal(u_g, u_big[:nb]) and np.array_equal(ts_g, ts_big[:nb]), nb
        for lo in (0, 50, 100, 150, h - 25, B - 50):                           # one-pass form (below one wavefront of rows)
            u_s, ts_s = be.osc(p, q[lo:lo + 50], dq[lo:lo + 50], t[lo:lo + 50])
            assert np.array_equal(u_s, u_big[lo:lo + 50]) and np.array_equal(ts_s, ts_big[lo:lo + 50]), lo
        # no training signal among the outputs (the NOTS instantiations): the same u, bit for bit, in every form
        u_nots = be.e.osc_generate(be.arm_id, 6, p, q, dq, t)
        u_nots_h = np.concatenate([be.e.osc_generate(be.arm_id, 6, p, q[:h], dq[:h], t[:h]),
                                   be.e.osc_generate(be.arm_id, 6, p, q[h:], dq[h:], t[h:])])
        assert np.array_equal(u_nots, u_nots_h)
        assert np.array_equal(be.e.osc_generate(be.arm_id, 6, p, q[:50], dq[:50], t[:50]), u_nots[:50])
        # one call cut into uneven shards: 16 shards of ~4100 rows (hand-over), 1500 shards of ~43 rows (one-pass)
        for n_sh in (16, 1500):
            u_sh, ts_sh = engine.osc_generate_sharded(be.arm_id, 6, p, q, dq, t, [0] * n_sh, training_signal=True)
            assert np.array_equal(u_sh, u_big) and np.array_equal(ts_sh, ts_big), n_sh
        # (random rows: the near-singular postures in front are conditioned up to 1e13 - their own tests gate on that)
        uo, _ = cases.OracleBackend("ur5").osc(p, q[300:1800], dq[300:1800], t[300:1800])
        assert np.percentile(cases.rel_err(u_big[300:1800], uo), 99) < 1e-9


_OBS_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from abr_control_amd import _abi
from tests import cases
d = np.load(sys.argv[2], allow_pickle=True)
out = {}
for arm in ("ur5", "threejoint"):
    be = cases.GpuBackend(arm)
    q = d["q_" + arm]
    for i in range(int(d["n_sets"])):
        P = _abi.make_obstacles_params(d[f"obs{i}"].tolist(), float(d[f"thr{i}"]), 30)
        out[f"{arm}_{i}_f64"] = be.obstacles(P, q)
        out[f"{arm}_{i}_f32"] = be.obstacles(P, q, dtype=np.float32)
np.savez(sys.argv[3], **out)
"""


def test_gpu_obstacles_redistributed_pairs_equal_one_pass_kernel(tmp_path):
    """obstacles_lds_kernel (the heavy pairs of a wavefront's 64 rows spread over its lanes through LDS) against the
    one-pass kernel (measurement switch ABRK_OBS_PLAIN) and the oracle: 1 / 3 / 16 obstacles, every pair near (more pairs
    than the wavefront's list holds: the overflow stays with its row), a batch that is not a multiple of 64, fp64 and
    fp32"""
    import subprocess
    import sys

    from tests.conftest import REPO

    rng = np.random.RandomState(8)
    sets = [([[0.3, 0.2, 0.4, 0.1], [-0.2, 0.4, 0.3, 0.05], [0.1, -0.3, 0.6, 0.15]], 0.3),
            ([[0.25, 0.1, 0.5, 0.1]], 0.4),
            ((rng.uniform(-0.6, 0.6, (16, 4)) * [1, 1, 1, 0.2] + [0, 0, 0.4, 0.12]).tolist(), 0.3),
            ((rng.uniform(-0.6, 0.6, (16, 4)) * [1, 1, 1, 0.1] + [0, 0, 0.4, 0.06]).tolist(), 5.0)]
    data = dict(n_sets=len(sets), q_ur5=rng.uniform(0, 2 * np.pi, (5003, 6)), q_threejoint=rng.uniform(0, 2 * np.pi, (5003, 3)))
    for i, (obs, thr) in enumerate(sets):
        data[f"obs{i}"], data[f"thr{i}"] = np.array(obs), thr
    np.savez(tmp_path / "in.npz", **data)
    (tmp_path / "run.py").write_text(_OBS_SCRIPT)
    res = {}
    for name, sw in (("lds", {}), ("plain", dict(ABRK_MEASUREMENT="1", ABRK_OBS_PLAIN="1"))):
        env = {k: v for k, v in os.environ.items() if k not in ("ABRK_OBS_PLAIN", "ABRK_MEASUREMENT")}
        env.update(sw)
        r = subprocess.run([sys.executable, str(tmp_path / "run.py"), REPO, str(tmp_path / "in.npz"),
                            str(tmp_path / f"{name}.npz")], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        res[name] = np.load(tmp_path / f"{name}.npz")
    for k in res["lds"].files:
        a, b = res["lds"][k].astype(float), res["plain"][k].astype(float)
        assert np.all(np.isfinite(a)), k
        tol = 1e-11 if k.endswith("f64") else 2e-3
        assert np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b))), (k, np.max(np.abs(a - b)))
    # and the oracle (rows the reference itself inverts noise on are left out: its mobility diagnostic)
    from oracle.oracle import Oracle

    P = _abi.make_obstacles_params(sets[0][0], sets[0][1], 30)
    uo, diag = Oracle(_abi.load_table("ur5")).avoid_obstacles_batch(P, data["q_ur5"][:600])
    ok = (diag[:, 0] > 1e-7) & (diag[:, 1] > 1e-20)
    err = np.max(np.abs(res["lds"]["ur5_0_f64"][:600] - uo), axis=1) / np.maximum(np.max(np.abs(uo), axis=1), 1e-9)
    assert err[ok].max() <= 1e-6


def test_gpu_table_sincos_negative_and_large_angles():
    """the OSC / Sliding kernels take sin/cos through the 128-entry LDS table (abrk_sincos_table.h): negative angles,
    angles up to the routine's range (|q| < 1e5; beyond it the library path), fp64 and fp32, builtin and user arms,
    against the oracle (libm)"""
    from oracle.oracle import Oracle

    o = Oracle(_abi.load_table("ur5"))
    rng = np.random.RandomState(123)
    B = 4000
    dq, t = rng.uniform(-2, 2, (B, 6)), rng.uniform(-0.8, 0.8, (B, 6))
    p = _abi.make_osc_params(6, kp=200, use_C=True)
    for scale in (7.0, 1e3, 9.9e4, 3e5):
        q = rng.uniform(-scale, scale, (B, 6))
        q[0] = 0.0
        q[1] = -np.pi / 128 * np.arange(1, 7)          # table nodes and half-way points
        q[2] = np.pi / 256 * (2 * np.arange(1, 7) + 1)
        uo = o.osc_batch(p, q, dq, t)
        for variant in ("static", "rt"):
            u = cases.GpuBackend("ur5", variant).osc(p, q, dq, t)[0]
            err = cases.rel_err(u, uo)
            # sin/cos of |q| ~ 1e5 are only defined to ~1e-11 (ulp of the argument); the law amplifies by cond(Mx)
            tol_med, tol_max = (1e-12, 1e-7) if scale <= 1e3 else (1e-9, 1e-4)
            assert np.median(err) <= tol_med and np.percentile(err, 99) <= tol_max, (scale, variant, np.median(err), err.max())
    # fp32 Sliding (config 5's kernel) on negative / moderately large angles vs its fp64 twin
    be = cases.GpuBackend("threejoint")
    sp = _abi.make_sliding_params(3)
    q3, dq3, t3 = rng.uniform(-300, 300, (B, 3)), rng.uniform(-2, 2, (B, 3)), rng.uniform(-1, 1, (B, 3))
    u64 = be.sliding(sp, q3, dq3, t3)[0]
    u32 = be.sliding(sp, q3.astype(np.float32), dq3.astype(np.float32), t3.astype(np.float32), dtype=np.float32)[0]
    q32 = q3.astype(np.float32).astype(float)  # the fp32 kernel sees rounded angles: compare on the same inputs
    u64r = be.sliding(sp, q32, dq3.astype(np.float32).astype(float), t3.astype(np.float32).astype(float))[0]
    well = (np.abs(np.sin(q32[:, 1])) > 0.05) & (np.abs(np.sin(q32[:, 2])) > 0.05)
    assert np.median(cases.rel_err(u32.astype(float), u64r)[well]) < 2e-5
    assert np.isfinite(u64).all()


def test_gpu_closed_loop_as_recorded_plan_matches_fused_rollout():
    """the examples' loop (examples/PyGame/force_osc_xy.py:57-78) as a recorded two-kernel tick - OSC.generate, then the
    plant step advancing q, dq in place - replayed 300 times as hipGraph launches, against the fused rollout kernel and
    the reference's own loop (tests/golden/twojoint.npz rollout_*)"""
    import abr_control_amd as a
    from abr_control_amd import engine
    from abr_control_amd.arms import twojoint
    from abr_control_amd.arms.twojoint import ArmSim
    from abr_control_amd.controllers import OSC, Damping, RestingConfig

    g = golden("twojoint")
    rc = twojoint.Config()
    q0, dq0, tgt = g["rollout_q0"], g["rollout_dq0"], g["rollout_target"]
    T = int(g["rollout_T"])
    ctrlr = OSC(rc, kp=20, use_C=True, ctrlr_dof=cases.XY, null_controllers=[
        Damping(rc, kv=10), RestingConfig(rc, kp=50, kv=np.sqrt(50), rest_angles=[np.pi / 4, np.pi])])
    sim = ArmSim(rc, dt=0.001, q_init=q0.copy())
    sim.dq = dq0.copy()
    sim.rollout(ctrlr, tgt, T)
    s = a.Stream(0)
    qd, dqd, td = _dev(q0, dq0, tgt)
    u = a.DeviceArray((len(q0), 2))
    with engine.Plan(0, s) as tick:
        engine.osc_generate(rc.arm_id, 2, ctrlr._params("EE", None), qd, dqd, td, u=u, stream=s)
        engine.twolink_step(sim._plant, qd, dqd, u, stream=s)
    for _ in range(T // 100):
        tick.launch_graph(100)
    s.sync()
    # same arithmetic, different fusion: equal to rounding accumulated over 300 steps
    assert np.max(np.abs(qd.numpy() - sim.q)) < 1e-9 and np.max(np.abs(dqd.numpy() - sim.dq)) < 1e-8
    assert np.max(np.abs(qd.numpy() - g["rollout_qD"][:, -1])) < 1e-9  # the reference's loop (fp64 formulas), last checkpoint


def test_gpu_compiled_user_arm_equals_the_builtin_bit_for_bit():
    """a user arm's compiled kernels (specialize.py, abrk_arm_create_compiled) are the StaticArm instantiations a
    built-in arm gets: the built-in threejoint's table, registered as a user arm with its plugin, returns the built-in's
    bits - dynamics, the OSC law and BASELINE config 5's Sliding law in both arithmetic types"""
    from tests import compiled_arms

    tab = compiled_arms.test_arms()["threejoint_user"]
    cu, bi = cases.GpuBackend(tab, "compiled"), cases.GpuBackend("threejoint")
    q, dq, t = draw(31, 5000, 3)
    for dtype in (np.float64, np.float32):
        a = cu.dynamics(q, dq, "EE", [0.1, -0.2, 0.05], ("Tx", "J", "dJ", "M", "g", "C", "R", "quat"), dtype=dtype)
        b = bi.dynamics(q, dq, "EE", [0.1, -0.2, 0.05], ("Tx", "J", "dJ", "M", "g", "C", "R", "quat"), dtype=dtype)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        for p in (_abi.make_osc_params(3, kp=50), _abi.make_osc_params(3, kp=50, use_C=True, ctrlr_dof=[1, 1, 0, 0, 0, 1],
                                                                       null_controllers=[_abi.make_damping(5)])):
            assert np.array_equal(cu.osc(p, q, dq, t, dtype=dtype)[0], bi.osc(p, q, dq, t, dtype=dtype)[0])
        sp = _abi.make_sliding_params(3)
        ua, ub = cu.sliding(sp, q, dq, t[:, :3], dtype=dtype), bi.sliding(sp, q, dq, t[:, :3], dtype=dtype)
        assert np.array_equal(ua[0], ub[0]) and np.array_equal(ua[1], ub[1])


def test_gpu_compiled_user_arm_against_the_oracle_and_the_runtime_table_kernels():
    """an arm no built-in resembles (4 joints, non-orthogonal fixed rotations): its compiled kernels against the oracle
    at the north_star bound and against the runtime-table kernels of the same table (both fp64: 1e-11), through the
    engine and through the robot_config / controller classes, recorded plans included"""
    import abr_control_amd as a
    from abr_control_amd import arms, engine
    from abr_control_amd.controllers import OSC, Damping
    from oracle.oracle import Oracle
    from tests import compiled_arms

    tab = compiled_arms.test_arms()["synthetic4"]
    cu, rt, o = cases.GpuBackend(tab, "compiled"), cases.GpuBackend(tab), Oracle(tab)
    rng = np.random.RandomState(5)
    B = 400
    q, dq, t = rng.uniform(-3, 3, (B, 4)), rng.uniform(-2, 2, (B, 4)), rng.uniform(-0.5, 0.5, (B, 6))
    want = ("Tx", "J", "dJ", "M", "g", "C", "R", "quat", "T", "Tinv")
    for frame, off in (("EE", [0.05, -0.02, 0.03]), ("link2", None), ("joint3", [0.0, 0.1, 0.0])):
        r, r2 = cu.dynamics(q, dq, frame, off, want), rt.dynamics(q, dq, frame, off, want)
        for k in want:
            assert np.allclose(r[k], r2[k], atol=1e-11), (frame, k)
        for b in range(0, B, 13):
            assert np.allclose(r["Tx"][b], o.Tx(frame, q[b], off), atol=1e-12)
            assert np.allclose(r["J"][b], o.J(frame, q[b], off), atol=1e-12)
            assert np.allclose(r["dJ"][b], o.dJ(frame, q[b], dq[b], off), atol=1e-11)
            assert np.allclose(r["M"][b], o.M(q[b]), atol=1e-12) and np.allclose(r["g"][b], o.g(q[b]), atol=1e-12)
            assert np.allclose(r["C"][b], o.C(q[b], dq[b]), atol=1e-11)
            assert np.allclose(r["quat"][b], o.quaternion(frame, q[b]), atol=1e-10)
    ok = np.array([np.linalg.cond(o.M(q[b])) < 1e8 for b in range(B)])
    P = _abi.make_osc_params
    for p in (P(4, kp=30), P(4, kp=30, use_C=True, null_controllers=[_abi.make_damping(3)]),
              P(4, kp=30, ko=20, ctrlr_dof=[1, 1, 1, 1, 0, 0], vmax=[0.5, 1.0])):
        u, ts = cu.osc(p, q, dq, t)
        uo = o.osc_batch(p, q, dq, t)
        assert cases.rel_err(u, uo)[ok].max() < 1e-6
        assert cases.rel_err(u, rt.osc(p, q, dq, t)[0])[ok].max() < 1e-9
    us = cu.sliding(_abi.make_sliding_params(4), q, dq, t[:, :3])[0]
    assert cases.rel_err(us, rt.sliding(_abi.make_sliding_params(4), q, dq, t[:, :3])[0]).max() < 1e-8
    # the classes: the cached plugin is picked up without being asked for; compiled=False keeps the runtime table
    rc, rc_rt = arms.from_table(tab), arms.from_table(tab, compiled=False)
    assert rc.plugin_path and rc_rt.plugin_path is None
    ctrl = OSC(rc, kp=30, null_controllers=[Damping(rc, kv=3)], use_C=True)
    ctrl_rt = OSC(rc_rt, kp=30, null_controllers=[Damping(rc_rt, kv=3)], use_C=True)
    uc = ctrl.generate(q, dq, t)
    assert cases.rel_err(uc, ctrl_rt.generate(q, dq, t))[ok].max() < 1e-9
    assert cases.rel_err(uc, o.osc_batch(P(4, kp=30, use_C=True, null_controllers=[_abi.make_damping(3)]), q, dq, t))[ok].max() < 1e-6
    assert np.allclose(rc.M(q[3]), o.M(q[3]).astype(np.float32)) and rc.M(q[3]).dtype == np.float32
    # a recorded plan on a compiled arm carries no table copy and replays as a graph
    s = a.Stream(0)
    qd, dd, td = (a.DeviceArray.from_numpy(x) for x in (q, dq, t))
    ud = a.DeviceArray((B, 4))
    with engine.Plan(0, s) as plan:
        engine.osc_generate(rc.arm_id, 4, P(4, kp=30), qd, dd, td, u=ud, stream=s)
    plan.launch_graph(3)
    s.sync()
    assert np.array_equal(ud.numpy(), cu.osc(P(4, kp=30), q, dq, t)[0])
    plan.close()


def test_gpu_concurrent_threads_own_streams():
    """include/abrk.h: entry points are re-entrant per (device, stream).  Eight host threads, each with its own stream,
    mix host-staged calls, device-resident calls, the six-row law with its deferred pass (worklists cached per stream),
    recording + replay of launch plans (the recorder is per thread) and user-arm registration / release (one registry) -
    every result must equal the single-threaded one bit for bit"""
    import ctypes as C
    import threading

    import abr_control_amd as a
    from abr_control_amd import engine
    from abr_control_amd._lib import check, lib

    arm = check(lib().abrk_arm_builtin(b"ur5"))
    P3, P6 = _abi.make_osc_params(6, kp=200, use_C=True), _abi.make_osc_params(6, kp=100, ko=80, ctrlr_dof=[1] * 6)
    desc = _abi.desc_from_table(_abi.load_table("jaco2"))
    n_threads, rounds = 8, 12
    inputs = [draw(100 + k, 20000 + 64 * k, 6) for k in range(n_threads)]
    expect = [(engine.osc_generate(arm, 6, P3, *inputs[k]), engine.osc_generate(arm, 6, P6, *inputs[k]))
              for k in range(n_threads)]
    errors = []

    def work(k):
        try:
            q, dq, t = inputs[k]
            s = a.Stream(0)
            qd, dd, td = (a.DeviceArray.from_numpy(x) for x in (q, dq, t))
            u3, u6 = a.DeviceArray(q.shape), a.DeviceArray(q.shape)
            for r in range(rounds):
                # host arrays in and out (per-thread staging), on this thread's stream
                assert np.array_equal(engine.osc_generate(arm, 6, P3, q, dq, t, stream=s), expect[k][0])
                # device-resident, six rows: deferred second pass with this stream's worklist
                engine.osc_generate(arm, 6, P6, qd, dd, td, u=u6, stream=s)
                # a plan recorded and replayed by this thread while the others record theirs
                with engine.Plan(0, s) as plan:
                    engine.osc_generate(arm, 6, P3, qd, dd, td, u=u3, stream=s)
                    engine.osc_generate(arm, 6, P6, qd, dd, td, u=u6, stream=s)
                plan.launch()
                plan.launch_graph(2)
                s.sync()
                assert np.array_equal(u3.numpy(), expect[k][0]) and np.array_equal(u6.numpy(), expect[k][1])
                plan.close()
                # the arm registry under contention
                uid = check(lib().abrk_arm_create(C.byref(desc)))
                assert uid >= 5
                um = engine.dynamics(uid, 6, q[:64], None, _abi.frame_id("EE", 6), None, ("M",), np.float64, 0, s)["M"]
                assert np.isfinite(um).all()
                assert lib().abrk_arm_destroy(uid) == 0
        except BaseException as e:  # noqa: BLE001 - reported on the main thread
            errors.append((k, repr(e)))

    ths = [threading.Thread(target=work, args=(k,)) for k in range(n_threads)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors, errors


def test_gpu_three_row_law_near_singular_postures():
    """the x,y,z law where Mx_inv is nearly singular (elbow stretched / folded to 1e-2 .. 1e-9 rad): the cofactor form
    of Mx hands over to the Cholesky factor there (osc_law's accuracy gate) and the truncating pinv takes most rows"""
    worst, beyond, trunc = cases.check_near_singular_postures(cases.GpuBackend("ur5"))
    assert beyond > 100 and trunc > 100, (beyond, trunc)
    assert worst < 1e-6
