"""The six-row law (all six task rows: `osc6` / `osc5_j2` on the bench line) at the batch sizes where its launch form
changes (csrc/abrk_osc6_plan.h osc6_plan - tests/test_osc6_plan.py holds it to this table -, abrk_kernels.h
Launch::osc_launch):

    rows                  form
    < 64                  one pass (`osc_kernel<.., PASS = 0>`, mode 0)
    64 - 65 536           first pass (mode 1) + per-chunk or grouped finish kernel on hand-over records
    65 537 - 1 048 576    first pass (mode 1) + dense finish kernel (abrk_finish.h osc6_finish_dense_kernel)
    > 1 048 576           first pass (mode 1) + recompute pass over the worklist (`PASS = 0`, mode 2)

The first pass of every kernel other than the plain law's two-waves-per-SIMD form is a persistent grid of at most
kKm6GridCap = 4096 blocks: beyond 262 144 rows its wavefronts loop, recording one deferral mask per step.

A row's bits do not depend on the batch it arrives in: every large call is compared bit for bit with the
one-pass form (calls of at most 48 rows) on windows of its rows - u, training signal and integral state - and with the
CPU oracle on a sample.  Inputs: the reference benchmark's random states plus two blocks of postures next to the arm's
kinematic singularities (tests/cases.py near_singular_postures, tiled three times): one inside a single 4096-row group of
the dense finish kernel (more than 256 deferring rows there: its wavefronts loop), one at the very end of the batch (the
partial last chunk).  `-m gpu` only."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from abr_control_amd import _abi
from tests import cases

pytestmark = pytest.mark.gpu

GROUP = 4096  # rows of one group of the dense finish kernel (64 chunks of 64 rows)
WIN = cases.GpuBackend.ONE_PASS_ROWS  # rows of a one-pass call
GRID_ROWS = 4096 * 64  # kKm6GridCap blocks of 64 rows: where a persistent first pass starts its second iteration
DENSE_TOP = 1 << 20  # Osc6Switches::dense_max: the largest batch of the dense finish form
SIX = cases.SIX

# the six-row settings of the existing suite (bench.py osc6 / osc5_j2, cases.check_six_row_near_singular,
# test_gpu_six_row_deferred_pass_equals_inline_sweeps).  ts: whether the call asks for the training signal
CTRL = {
    # (a) the plain law: on UR5 the NOTS and EEF instantiations the bench times
    "plain": dict(kw=dict(kp=200, ko=150, kv=25, ctrlr_dof=SIX), ts=True),
    "plain_nots": dict(kw=dict(kp=200, ko=150, kv=25, ctrlr_dof=SIX), ts=False),
    # (b) a masked row (every row defers), orientation algorithm 1, Coriolis term, a fused null controller
    "masked_C_null": dict(kw=dict(kp=100, ko=60, kv=12, ctrlr_dof=[1, 0, 1, 1, 1, 0], orientation_algorithm=1, use_C=True,
                                  null_controllers=[_abi.make_damping(5)]), ts=True),
    # (c) integral term over two steps, target velocity, external null-space signal
    "ki_tv_ext": dict(kw=dict(kp=100, ko=60, kv=12, ki=0.2, ctrlr_dof=SIX, vmax=[0.5, 1.0], use_g=False), ts=True,
                      tv=True, ext=True, steps=2),
    # (d) Jaco2: five rows (bench.py osc5_j2) and the Coriolis term
    "j2_five": dict(kw=dict(kp=200, ctrlr_dof=[1] * 5 + [0]), ts=False),
    "j2_C": dict(kw=dict(kp=100, ko=60, kv=12, ctrlr_dof=SIX, use_C=True), ts=True),
}


def _ctrls(arm, names):
    return [c for c in names if arm == "jaco2" or not c.startswith("j2_")]


_NS = {}


def _near_singular(arm):
    """near_singular_postures(arm, 600) tiled three times (one block), and per row of the block the six-row gate
    (cases.six_row_gate) of every controller's task rows, from the oracle - computed once per arm"""
    if arm not in _NS:
        from oracle.oracle import Oracle

        o = Oracle(_abi.load_table(arm))
        qs = cases.near_singular_postures(arm, 600)
        gates = {}
        for dof in {tuple(c["kw"]["ctrlr_dof"]) for c in CTRL.values()}:
            ok, trunc, cond = cases.six_row_gate(o, qs, list(dof))
            gates[dof] = (np.tile(ok, 3), np.tile(trunc, 3), np.tile(cond, 3))
        _NS[arm] = (np.tile(qs, (3, 1)), gates)
    return _NS[arm]


def _inputs(arm, B, dtype, qs, seed=1):
    """random states (examples/timing_plots.py:18-20) + target velocity + external null-space signal; the near-singular
    block `qs` in the middle of one 4096-row group and again at the very end of the batch.
    -> (inputs, indices of the near-singular rows, first row of the group that holds the middle block)"""
    n = 6
    rng = np.random.RandomState(seed)
    d = dict(q=rng.uniform(0, 2 * np.pi, (B, n)), dq=rng.uniform(0, 5, (B, n)), t=rng.uniform(-1, 1, (B, 6)),
             tv=rng.uniform(-0.5, 0.5, (B, 6)), une=rng.uniform(-2, 2, (B, n)))
    L = len(qs)
    assert L <= GROUP and 2 * L + GROUP <= B
    g0 = (B // 2) // GROUP * GROUP
    mid = g0 + (GROUP - L) // 2
    d["q"][mid:mid + L] = qs
    d["q"][B - L:] = qs
    ns = np.r_[mid:mid + L, B - L:B]
    return {k: np.ascontiguousarray(v, dtype) for k, v in d.items()}, ns, g0


def _call(arm_id, c, d, lo, hi, dtype):
    """the controller `c` on rows [lo, hi) of the inputs `d`, `steps` times (only the integral state evolves) ->
    per step {"u", "ts", "ie"} (None where absent)"""
    from abr_control_amd import engine

    p = _abi.make_osc_params(6, **c["kw"])
    sl = slice(lo, hi)
    ie = np.zeros((hi - lo, 6), dtype) if p.ki != 0 else None
    out = []
    for _ in range(c.get("steps", 1)):
        r = engine.osc_generate(arm_id, 6, p, d["q"][sl], d["dq"][sl], d["t"][sl], d["tv"][sl] if c.get("tv") else None,
                                ie, d["une"][sl] if c.get("ext") else None, training_signal=c["ts"], dtype=dtype)
        u, ts = r if c["ts"] else (r, None)
        out.append(dict(u=u, ts=ts, ie=None if ie is None else ie.copy()))
    return out


def _windows(B, ns, rng, extra=12):
    """first rows of the one-pass windows: row 0, both sides of row 262 144 and of row 1 048 576, every near-singular row,
    the last WIN rows, `extra` at random"""
    starts = {0, B - WIN}
    for edge in (GRID_ROWS, DENSE_TOP):
        starts |= {edge - WIN, edge - WIN // 2, edge}
    for lo, hi in ((ns[0], ns[len(ns) // 2 - 1] + 1), (ns[len(ns) // 2], ns[-1] + 1)):
        starts |= set(range(lo, hi, WIN))
    starts |= set(rng.randint(0, B - WIN, extra).tolist())
    return sorted(s for s in starts if 0 <= s <= B - WIN)


def _check_large_call(arm, variant, dtype, B, ctrl_names, seed=1):
    """every controller of `ctrl_names` on one B-row batch: bit-equal to the one-pass form on windows, within TOL_D (fp64)
    / TOL_F32 (fp32, well-conditioned rows) of the oracle on a sample and on the gated near-singular rows, integral
    state within 1e-9 of the oracle's after two steps, finite wherever the oracle is"""
    from oracle.oracle import Oracle

    be = cases.GpuBackend(arm, variant)
    o = Oracle(_abi.load_table(arm))
    qs, gates = _near_singular(arm)
    d, ns, g0 = _inputs(arm, B, dtype, qs, seed)
    # the middle block really fills one dense-finish group with more than 256 truncating rows (4 wavefronts x 64
    # records: the `w += gridDim.y` loop runs)
    in_group = (ns >= g0) & (ns < g0 + GROUP)
    assert in_group.sum() == len(qs) and gates[tuple(SIX)][1].sum() > 256, gates[tuple(SIX)][1].sum()
    rng = np.random.RandomState(B % 9973)
    wins = _windows(B, ns, rng)
    others = np.setdiff1d(np.arange(B), ns)
    sample = np.sort(rng.choice(others, 1500, replace=False))
    f32 = dtype == np.float32
    tol = cases.TOL_F32 if f32 else cases.TOL_D
    d64 = {k: np.asarray(v, float) for k, v in d.items()}
    for name in ctrl_names:
        c = CTRL[name]
        dof = tuple(c["kw"]["ctrlr_dof"])
        big = _call(be.arm_id, c, d, 0, B, dtype)
        # ---- bit for bit against the one-pass form
        for lo in wins:
            w = _call(be.arm_id, c, d, lo, lo + WIN, dtype)
            for s, (bs, ws) in enumerate(zip(big, w)):
                for k in ("u", "ts", "ie"):
                    if bs[k] is not None:
                        assert np.array_equal(bs[k][lo:lo + WIN], ws[k], equal_nan=True), \
                            f"{arm}-{variant} {np.dtype(dtype).name} B={B} {name}: {k} of step {s + 1}, rows {lo}..{lo + WIN} " \
                            f"differ from the one-pass form"
        # ---- against the oracle: the sample (gated like the near-singular rows) and the gated near-singular rows
        ok_s, trunc_s, cond_s = cases.six_row_gate(o, d64["q"][sample], list(dof))
        ok_n, trunc_n, cond_n = (np.tile(x, 2) for x in gates[dof])  # (the two blocks)
        rows = np.r_[sample, ns]
        ok, trunc, cond = np.r_[ok_s, ok_n], np.r_[trunc_s, trunc_n], np.r_[cond_s, cond_n]
        # fp32: TOL_F32 on rows with cond(Mx_inv) < 1e3 (test_gpu_bench_workloads_match_the_oracle), and - six rows mix
        # metres and radians, their cond starts near 1e3: on UR5 no random row is below it - 2e-7 cond (about 3 fp32
        # roundings, amplified by the conditioning) on every row up to cond 1e6 that does not truncate
        wide = ok & (cond < 1e6) & ~trunc
        if f32:
            ok &= cond < 1e3
            assert wide[:len(sample)].sum() > 0.5 * len(sample), (name, wide[:len(sample)].sum())
        else:
            assert ok[:len(sample)].sum() > 0.9 * len(sample), (name, ok[:len(sample)].sum())
            assert ok[len(sample):].sum() > len(ns) // 3, (name, ok[len(sample):].sum())
        p = _abi.make_osc_params(6, **c["kw"])
        ie_o = np.zeros((len(rows), 6)) if p.ki != 0 else None
        for s, bs in enumerate(big):
            uo, tso = o.osc_batch(p, d64["q"][rows], d64["dq"][rows], d64["t"][rows],
                                  d64["tv"][rows] if c.get("tv") else None, ie_o, d64["une"][rows] if c.get("ext") else None,
                                  want_training=True)
            u = np.asarray(bs["u"][rows], float)
            fin = np.isfinite(uo).all(axis=1)
            assert np.isfinite(u[fin]).all(), f"{arm} B={B} {name}: non-finite u where the oracle's is finite"
            rel = cases.rel_err(u, uo)
            err = rel[ok] if ok.any() else np.zeros(1)
            assert err.max() <= tol, f"{arm}-{variant} {np.dtype(dtype).name} B={B} {name} step {s + 1}: {err.max():.3e}"
            if f32:
                bad = rel[wide] > np.maximum(tol, 2e-7 * cond[wide])
                assert not bad.any(), f"{arm} f32 B={B} {name} step {s + 1}: error above 2e-7 cond on {bad.sum()} rows"
            if bs["ts"] is not None and not f32:
                errt = cases.rel_err(np.asarray(bs["ts"][rows], float), tso)[ok]
                assert errt.max() <= tol, f"{arm} B={B} {name} step {s + 1}: training signal {errt.max():.3e}"
            if ie_o is not None:
                assert np.allclose(bs["ie"][rows], ie_o, rtol=1e-9 if not f32 else 1e-5, atol=1e-12 if not f32 else 1e-6), \
                    f"{arm} B={B} {name} step {s + 1}: integrated_error"


# ---------------------------------------------------------------------------- 1. the recompute form (> 1 M rows)
@pytest.mark.parametrize("B", [DENSE_TOP + 1, DENSE_TOP + 12_325], ids=["1M+1", "1M+12325"])
@pytest.mark.parametrize("arm,variant,dtype", [("ur5", "static", np.float64), ("ur5", "rt", np.float64),
                                               ("jaco2", "static", np.float64), ("ur5", "static", np.float32)],
                         ids=["ur5-static-f64", "ur5-rt-f64", "jaco2-static-f64", "ur5-static-f32"])
def test_gpu_six_row_recompute_form(arm, variant, dtype, B):
    """beyond 1 048 576 rows the deferred rows are not handed over: the first pass parks their indices in a worklist and
    a second launch of the complete row program (`PASS = 0`, mode 2) evaluates them again - the pass that would leave
    them with whatever `u` held if it were not launched, and that must not integrate a deferred row's error twice.  One
    row in the last chunk / a partial last chunk; every controller; the plain law with and without the training signal
    (UR5: the NOTS and EEF instantiations)"""
    names = ["plain", "plain_nots", "masked_C_null", "ki_tv_ext"] + (["j2_five", "j2_C"] if arm == "jaco2" else [])
    _check_large_call(arm, variant, dtype, B, names)


# ---------------------------------------------------------------------------- 2. non-plain kernels, 262 144 .. 1 M rows
@pytest.mark.parametrize("B", [GRID_ROWS, GRID_ROWS + 1, 300_037, DENSE_TOP - 17])
@pytest.mark.parametrize("arm,variant", [("ur5", "static"), ("ur5", "rt"), ("jaco2", "static")])
def test_gpu_six_row_persistent_grid_handover_band(arm, variant, B):
    """the kernels whose first pass is a persistent grid (Coriolis term, fused null controllers, integral state / target
    velocity / external signal, Jaco2 with C: capped at kKm6GridCap = 4096 blocks) in the dense-finish band: beyond
    262 144 rows a wavefront loops in hand-over mode, noting its chunk's deferral mask at every step, and a deferred
    row stores its own integral state (abrk_rows.h) for the finish kernel, which never sees the row's inputs.  Windows
    on both sides of row 262 144, where block 0 starts its second iteration"""
    _check_large_call(arm, variant, np.float64, B, _ctrls(arm, ["masked_C_null", "ki_tv_ext", "j2_five", "j2_C"]))


# ---------------------------------------------------------------------------- 3. every form of the law, whole batches
_FORMS_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests import test_gpu_six_row_large_batches as m
m._forms_child(sys.argv[2], sys.argv[3])
"""

FORM_SWITCHES = (("default", {}),
                 ("recompute", dict(ABRK_DENSE_MAX="0")),  # recompute pass beyond 65 536 rows
                 ("dense", dict(ABRK_DENSE_MAX="4000000")),  # dense finish kernel beyond 1 M rows
                 ("no_handover", dict(ABRK_NO_HANDOVER="1")),  # first pass + recompute pass at every size here
                 ("handover_max", dict(ABRK_HANDOVER_MAX="262144")),  # 262 144 rows: the per-chunk finish kernel
                 ("onepass", dict(ABRK_NO_DEFER="1")))  # the complete row program, no second pass
FORM_SIZES = (GRID_ROWS, 300_037, DENSE_TOP + 12_325)
FORM_ARMS = (("ur5", np.float64), ("ur5", np.float32), ("jaco2", np.float64))
FORM_CTRLS = ("plain", "plain_nots", "masked_C_null", "ki_tv_ext")


def _digests(a):
    """one blake2b digest per 4096-row group of an output -> [groups, 16] uint8"""
    a = np.ascontiguousarray(a)
    return np.array([np.frombuffer(hashlib.blake2b(a[g:g + GROUP].tobytes(), digest_size=16).digest(), np.uint8)
                     for g in range(0, len(a), GROUP)])


def _forms_child(ns_path, out_path):
    """(child process, one set of measurement switches) every output of every (size, arm, dtype, controller) of the
    forms test, as digests per 4096-row group"""
    nsd = np.load(ns_path)
    out = {}
    for arm, dtype in FORM_ARMS:
        be = cases.GpuBackend(arm)
        for B in FORM_SIZES:
            d, _ns, _g0 = _inputs(arm, B, dtype, nsd[arm])
            for name in FORM_CTRLS:
                for s, st in enumerate(_call(be.arm_id, CTRL[name], d, 0, B, dtype)):
                    for k, v in st.items():
                        if v is not None:
                            out[f"{arm}|{np.dtype(dtype).name}|{B}|{name}|step{s + 1}|{k}"] = _digests(v)
    np.savez(out_path, **out)


def test_gpu_six_row_forms_agree_bitwise_on_large_batches(tmp_path):
    """the measurement switches that choose between the six-row forms (ABRK_DENSE_MAX,
    ABRK_HANDOVER_MAX, ABRK_NO_HANDOVER, ABRK_NO_DEFER; read once per process, only under ABRK_MEASUREMENT=1) leave every
    output unchanged to the bit - u, training signal and the integral state after each of two steps: 262 144 rows
    (where ABRK_HANDOVER_MAX moves the batch to the per-chunk finish kernel), 300 037 rows (the persistent first pass
    loops) and 1 M + 12 325 rows (recompute form by default); UR5 fp64 / fp32, Jaco2 fp64; the plain law with and
    without the training signal, a masked row + Coriolis + null controller, integral term + target velocity + external
    signal.  Each form in a child process of its own, compared through per-4096-row-group digests"""
    from tests.conftest import REPO

    np.savez(tmp_path / "ns.npz", **{arm: _near_singular(arm)[0] for arm, _ in FORM_ARMS})
    (tmp_path / "run.py").write_text(_FORMS_SCRIPT)
    res = {}
    for name, sw in FORM_SWITCHES:
        env = {k: v for k, v in os.environ.items() if not k.startswith(("ABRK_FINISH_", "ABRK_MEASUREMENT", "ABRK_NO_",
                                                                         "ABRK_DENSE_", "ABRK_HANDOVER_"))}
        if sw:
            env.update(sw, ABRK_MEASUREMENT="1")
        r = subprocess.run([sys.executable, str(tmp_path / "run.py"), REPO, str(tmp_path / "ns.npz"),
                            str(tmp_path / f"{name}.npz")], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, f"form {name}: exit {r.returncode}\n{r.stderr[-3000:]}"
        res[name] = dict(np.load(tmp_path / f"{name}.npz"))
    ref = res["default"]
    # u + ts (plain), u (plain_nots), u + ts (masked_C_null), u + ts + ie of each of two steps (ki_tv_ext)
    assert len(ref) == len(FORM_ARMS) * len(FORM_SIZES) * (2 + 1 + 2 + 2 * 3)
    bad = []
    for name, got in res.items():
        assert sorted(got) == sorted(ref), name
        for k, v in ref.items():
            diff = np.flatnonzero((got[k] != v).any(axis=1))
            if len(diff):
                bad.append(f"{name} vs default: {k}: groups {diff[:8].tolist()} (rows from {diff[0] * GROUP})")
    assert not bad, "\n".join(bad[:20])


# ---------------------------------------------------------------------------- 4. what the bench times, at its size
@pytest.mark.parametrize("workload", ["osc6", "osc5_j2"])
def test_gpu_bench_six_row_workloads_at_the_roofline_batch(workload):
    """bench.py's own `Runner` at the roofline batch (8 M rows: first pass + recompute pass), stepped through its recorded
    plan, against the oracle on 2000 rows and bit for bit against one-pass windows of the same rows (no training signal:
    the NOTS instantiations in every form)"""
    import abr_control_amd as a
    from abr_control_amd import engine
    from oracle.oracle import Oracle
    from tests.test_gpu_parity import _bench_module, _zero

    bench = _bench_module()
    st = a.Stream(0)
    r = bench.Runner(workload, 8 << 20, 0, st)
    _zero(r.u)  # (the constructor's untimed step has written u already)
    r.step()
    st.sync()
    u = r.u.numpy()
    q, dq, t = r.host
    B = r.B
    p = r.params
    rng = np.random.RandomState(3)
    for lo in sorted({0, GRID_ROWS - WIN // 2, DENSE_TOP - WIN // 2, B // 2, B - WIN} | set(rng.randint(0, B - WIN, 12).tolist())):
        w = engine.osc_generate(r.arm_id, r.n, p, q[lo:lo + WIN], dq[lo:lo + WIN], t[lo:lo + WIN], dtype=r.dt)
        assert np.array_equal(u[lo:lo + WIN], w, equal_nan=True), f"{workload}: rows {lo}..{lo + WIN}"
    o = Oracle(_abi.load_table(r.arm))
    rows = np.sort(rng.choice(B, 2000, replace=False))
    qr, dqr, tr = (np.asarray(x[rows], float) for x in (q, dq, t))
    uo = o.osc_batch(p, qr, dqr, tr)
    ok, _trunc, _cond = cases.six_row_gate(o, qr, list(p.ctrlr_dof))
    assert ok.sum() > 0.9 * len(rows)
    assert np.isfinite(u).all()
    err = cases.rel_err(np.asarray(u[rows], float), uo)[ok]
    assert err.max() <= cases.TOL_D, f"{workload} at {B} rows: {err.max():.3e} ({r.kernel_name()})"


def test_gpu_six_row_recompute_form_recorded_plan():
    """a (1 << 20) + 12 325-row UR5 call recorded as a plan on device arrays (its worklist is the plan's own): launch()
    writes what the direct call writes, bit for bit, and three hipGraph replays leave a stateless u unchanged; with an
    integral term two plan ticks equal two direct steps, integral state included"""
    import abr_control_amd as a
    from abr_control_amd import engine
    from tests.test_gpu_parity import _dev, _zero

    be = cases.GpuBackend("ur5")
    B = DENSE_TOP + 12_325
    d, _ns, _g0 = _inputs("ur5", B, np.float64, _near_singular("ur5")[0])
    s = a.Stream(0)
    qd, dqd, td, tvd, uned = _dev(d["q"], d["dq"], d["t"], d["tv"], d["une"])
    # stateless: the plain law, no training signal (bench.py's osc6)
    c = CTRL["plain_nots"]
    p = _abi.make_osc_params(6, **c["kw"])
    u_direct = _call(be.arm_id, c, d, 0, B, np.float64)[0]["u"]
    u = a.DeviceArray((B, 6))
    with engine.Plan(0, s) as plan:
        engine.osc_generate(be.arm_id, 6, p, qd, dqd, td, u=u, stream=s)
    _zero(u)
    plan.launch()
    s.sync()
    assert np.array_equal(u.numpy(), u_direct)
    _zero(u)
    plan.launch_graph(3)
    s.sync()
    assert np.array_equal(u.numpy(), u_direct)
    plan.close()
    # stateful: integral term + target velocity + external signal, two ticks
    c = CTRL["ki_tv_ext"]
    p = _abi.make_osc_params(6, **c["kw"])
    direct = _call(be.arm_id, c, d, 0, B, np.float64)
    ie = a.DeviceArray((B, 6))
    ts = a.DeviceArray((B, 6))
    _zero(ie)
    with engine.Plan(0, s) as plan:
        engine.osc_generate(be.arm_id, 6, p, qd, dqd, td, tvd, ie, uned, u=u, training_signal=ts, stream=s)
    for k in range(2):
        plan.launch()
        s.sync()
        assert np.array_equal(u.numpy(), direct[k]["u"]), f"tick {k + 1}: u"
        assert np.array_equal(ts.numpy(), direct[k]["ts"]), f"tick {k + 1}: training signal"
        assert np.array_equal(ie.numpy(), direct[k]["ie"]), f"tick {k + 1}: integrated_error"
    plan.close()
