"""C ABI and Python surface of the loop recorder (abrk_loop_trace_batch, engine.loop_trace, LoopRecorder): struct layout,
every rejection before any device use, the empty batch - no GPU needed; LoopRecorder's buffers and shapes on a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from abr_control_amd import _abi
from tests.conftest import REPO


def test_trace_params_layout_matches_header(tmp_path):
    src = r'''#include <stdio.h>
#include <stddef.h>
#include "abrk.h"
int main(){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d\n", sizeof(abrk_trace_params),
  offsetof(abrk_trace_params, frame), offsetof(abrk_trace_params, x_off), offsetof(abrk_trace_params, every),
  offsetof(abrk_trace_params, capacity), offsetof(abrk_trace_params, columns), offsetof(abrk_trace_params, tol),
  ABRK_TR_Q, ABRK_TR_DQ, ABRK_TR_U, ABRK_TR_TARGET, ABRK_TR_XYZ, ABRK_TR_ERR);return 0;}'''
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-o", exe], input=src.encode(),
                   check=True)
    v = [int(x) for x in subprocess.run([exe], capture_output=True, check=True).stdout.split()]
    P = _abi.TraceParams
    assert v[:7] == [C.sizeof(P), P.frame.offset, P.x_off.offset, P.every.offset, P.capacity.offset, P.columns.offset,
                     P.tol.offset]
    assert v[7:] == [_abi.TRACE_COLUMNS[k][0] for k in ("q", "dq", "u", "target", "xyz", "err")]
    p = _abi.make_trace_params(13, (1, 2, 3), every=4, capacity=5, columns=("err", "q"), tol=0.25)
    assert (p.frame, list(p.x_off), p.every, p.capacity, p.columns, p.tol) == (13, [1.0, 2.0, 3.0], 4, 5, 1 | 32, 0.25)
    assert _abi.trace_layout(p.columns, 6) == ({"q": (0, 6), "err": (6, 1)}, 7)
    assert _abi.trace_layout(63, 6)[1] == 28
    with pytest.raises(ValueError):
        _abi.trace_columns_mask(("xyz", "orientation"))
    with pytest.raises(ValueError):
        _abi.trace_columns_mask(("xyz", "xyz"))


def test_loop_trace_argument_validation_before_device():
    """every rejection of include/abrk.h's loop recorder section: ABRK_EINVAL, nothing launched (none needs a device)"""
    from abr_control_amd._lib import lib

    L = lib()
    assert L.abrk_version() == 100 and hasattr(L, "abrk_loop_trace_batch")
    B, n = 2, 6
    q, tg = np.zeros((B, n)), np.zeros((B, 6))
    counter, settle = np.zeros(B, np.int32), np.zeros(B, np.int32)
    hist, stats = np.zeros((3, B, 28)), np.zeros((B, 4))
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(p=None, arm=0, dtype=0, B=B, q=q, dq=q, u=q, target=tg, counter=counter, history=hist, stats=stats,
             settle=settle, **kw):
        if p is None:
            base = dict(frame=13, every=1, capacity=3, columns=63, tol=0.1)
            base.update(kw)
            p = _abi.make_trace_params(**base)
        rc = L.abrk_loop_trace_batch(arm, dtype, C.byref(p) if p is not False else None, B, vp(q), vp(dq), vp(u),
                                     vp(target), vp(counter), vp(history), vp(stats), vp(settle), 0, None)
        return rc, L.abrk_last_error().decode()

    bad = {
        "dtype": dict(dtype=7), "negative batch": dict(B=-1), "every": dict(every=0), "capacity": dict(capacity=0),
        "empty mask": dict(columns=0), "unknown mask": dict(columns=64 | 1), "q": dict(q=None), "dq": dict(dq=None),
        "u": dict(u=None), "target": dict(target=None), "settle": dict(settle=None),
        "neither": dict(history=None, stats=None), "frame low": dict(frame=-1), "frame high": dict(frame=14),
        "tol nan": dict(tol=np.nan), "tol inf": dict(tol=np.inf), "x_off nan": dict(x_off=(0, np.nan, 0)),
        "x_off inf": dict(x_off=(-np.inf, 0, 0)), "params": dict(p=False), "counter": dict(counter=None),
        # what only the statistics need, without a history
        "target for stats": dict(history=None, target=None), "q for stats": dict(history=None, q=None),
        "target for err": dict(stats=None, columns=32, target=None),
    }
    for what, kw in bad.items():
        rc, msg = call(**kw)
        assert rc == -1 and msg, (what, rc, msg)
    assert call(arm=999)[0] == -4
    # nothing was written by any of them
    assert not counter.any() and not hist.any() and not stats.any() and not settle.any()
    # sources that nothing selected needs may be NULL; a capacity / mask without a history is not looked at
    for kw in (dict(B=0), dict(B=0, dq=None, u=None, columns=1 | 8 | 16 | 32),
               dict(B=0, history=None, capacity=0, columns=0, dq=None, u=None),
               dict(B=0, stats=None, settle=None, columns=2, q=None, target=None, u=None)):
        rc, msg = call(**kw)
        assert rc == 0, (kw, msg)


def test_engine_loop_trace_checks_shapes_in_python():
    from abr_control_amd import engine

    p = _abi.make_trace_params(13, capacity=3, columns=63)
    q, tg, c = np.zeros((2, 6)), np.zeros((2, 6)), np.zeros(2, np.int32)
    with pytest.raises(ValueError):
        engine.loop_trace(0, 6, p, q, q, q, np.zeros((2, 3)), c, stats=np.zeros((2, 4)), settle=c.copy())
    with pytest.raises(ValueError):
        engine.loop_trace(0, 6, p, q, q, q, tg, c, history=np.zeros((3, 2, 27)))
    with pytest.raises(ValueError):
        engine.loop_trace(0, 6, p, q, q, q, tg, c.astype(np.int64), history=np.zeros((3, 2, 28)))
    with pytest.raises(ValueError):
        engine.loop_trace(0, 6, p, q, q, q, tg, c, stats=np.zeros((2, 4), np.float32), settle=c.copy())
    with pytest.raises(ValueError):
        engine.loop_trace(0, 6, p, None, None, None, None, c, stats=np.zeros((2, 4)), settle=c.copy())
    with pytest.raises(TypeError):
        engine.loop_trace(0, 6, p, q, q, q, tg, c, history=np.zeros((3, 2, 28)), dtype=np.float16)
    e, ce = np.zeros((0, 6)), np.zeros(0, np.int32)
    engine.loop_trace(0, 6, p, e, e, e, e, ce, history=np.zeros((3, 0, 28)))  # an empty batch: a no-op without a device


def test_loop_recorder_argument_checks():
    """everything LoopRecorder rejects, before it allocates anything"""
    import abr_control_amd as a
    from abr_control_amd.arms import ur5

    assert a.LoopRecorder is __import__("abr_control_amd.recorder", fromlist=["LoopRecorder"]).LoopRecorder
    rc = ur5.Config()
    for kw in (dict(B=0), dict(capacity=-1), dict(every=0), dict(capacity=0, stats=False), dict(tol=np.nan),
               dict(tol=np.inf), dict(capacity=4, columns=("xyz", "pose")), dict(capacity=4, columns=("err", "err")),
               dict(capacity=4, columns=()), dict(xyz_offset=(0, 1)), dict(xyz_offset=(0, np.nan, 0))):
        args = dict(B=8, capacity=0)
        args.update(kw)
        with pytest.raises(ValueError):
            a.LoopRecorder(rc, **args)
    with pytest.raises(Exception, match="Invalid transformation name"):
        a.LoopRecorder(rc, 8, ref_frame="link9")


@pytest.mark.gpu
def test_loop_recorder_buffers_and_shapes():
    import abr_control_amd as a
    from abr_control_amd.arms import ur5

    rc = ur5.Config()
    s = a.Stream(0)
    rec = a.LoopRecorder(rc, 70, capacity=5, every=2, columns=("err", "q", "xyz"), ref_frame="link3",
                         xyz_offset=(0, 0, 0.1), stream=s)
    assert rec.layout == {"q": (0, 6), "xyz": (6, 3), "err": (9, 1)} and rec.W == 10
    assert rec.device_history().shape == (5, 70, 10) and rec.device_history().dtype == np.float64
    ds = rec.device_stats()
    assert ds["stats"].shape == (70, 4) and ds["stats"].dtype == np.float64
    assert ds["settle"].shape == ds["counter"].shape == (70,) and ds["counter"].dtype == np.int32
    # before any tick: an empty history, NaN statistics, nobody settled
    h, st = rec.history(), rec.stats()
    assert {k: v.shape for k, v in h.items()} == {"q": (0, 70, 6), "xyz": (0, 70, 3), "err": (0, 70, 1)}
    assert np.isnan(st["err_rms"]).all() and not st["ticks"].any() and (st["settle_tick"] == -1).all()
    q, tg = a.DeviceArray((70, 6)).zero_(s), a.DeviceArray((70, 6)).zero_(s)
    for _ in range(3):
        rec.record(q, None, None, tg)
    h, st = rec.history(), rec.stats()
    assert h["xyz"].shape == (2, 70, 3) and not np.isnan(h["xyz"]).any()
    want = np.linalg.norm(rc.Tx("link3", np.zeros(6), x=[0, 0, 0.1]))
    assert np.allclose(st["err_last"], want, rtol=1e-12) and np.allclose(st["err_rms"], want, rtol=1e-12)
    assert (st["ticks"] == 3).all() and (st["settle_tick"] == -1).all()
    rec.reset(rows=(3, 9))
    assert np.array_equal(rec.stats()["ticks"] == 0, (np.arange(70) >= 3) & (np.arange(70) < 9))
    assert np.isnan(rec.history()["q"][:, 3:9]).all()
    # statistics only; history only
    so = a.LoopRecorder(rc, 8, stream=s)
    assert so.device_history() is None and so.device_stats()["stats"] is not None
    with pytest.raises(ValueError):
        so.history()
    ho = a.LoopRecorder(rc, 8, capacity=2, stats=False, stream=s)
    assert ho.device_stats()["stats"] is None and ho.device_stats()["settle"] is None
    with pytest.raises(ValueError):
        ho.stats()
    # an fp32 arm records an fp32 history and fp64 statistics
    r32 = a.LoopRecorder(ur5.Config(dtype=np.float32), 8, capacity=2, stream=s)
    assert r32.device_history().dtype == np.float32 and r32.device_stats()["stats"].dtype == np.float64
