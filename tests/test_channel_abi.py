"""The measurement channel without a GPU: the layout of abrk_channel_params / abrk_channel_state against the header,
every ABRK_EINVAL case of abrk_channel_step_batch (the checks come before the device is touched), the empty batch, and
the Python surface of sensing.SignalChannel / sensing.JointSensor - their arguments and what they refuse."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import abr_control_amd
from abr_control_amd import _abi, sensing
from abr_control_amd._lib import lib
from tests.conftest import REPO

W, B = 4, 3


def test_channel_structs_match_the_header(tmp_path):
    src = r'''#include <stdio.h>
#include <stddef.h>
#include "abrk.h"
#define O(f) offsetof(abrk_channel_params, f)
#define S(f) offsetof(abrk_channel_state, f)
int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(abrk_channel_params), O(width), O(delay), O(seed),
  O(row_offset), O(dt), O(tau_diff), O(bias), O(sigma), O(resolution));
  printf("%zu %zu %zu %zu %zu\n", sizeof(abrk_channel_state), S(counter), S(ring), S(prev), S(d_f));
  printf("%d %d\n", ABRK_CHANNEL_MAX_WIDTH, ABRK_CHANNEL_MAX_DELAY);return 0;}'''
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-o", exe], input=src.encode(),
                   check=True)
    lines = [[int(v) for v in ln.split()] for ln in
             subprocess.run([exe], capture_output=True, check=True).stdout.decode().splitlines()]
    P, S = _abi.ChannelParams, _abi.ChannelState
    assert lines[0] == [C.sizeof(P)] + [getattr(P, f).offset for f, _ in P._fields_] == [
        40 + 3 * 128, 0, 4, 8, 16, 24, 32, 40, 168, 296]
    assert lines[1] == [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_] == [32, 0, 8, 16, 24]
    assert lines[2] == [_abi.CHANNEL_MAX_WIDTH, _abi.CHANNEL_MAX_DELAY] == [16, 4096]


def test_the_entry_point_is_exported_and_the_version_stays():
    L = lib()
    assert L.abrk_version() == 100
    assert hasattr(L, "abrk_channel_step_batch")
    assert abr_control_amd.SignalChannel is sensing.SignalChannel and abr_control_amd.JointSensor is sensing.JointSensor


def _call(dtype=_abi.F64, B_=B, w0=W, w1=0, null=(), state_null=(), params=True, state=True, dy=False, cols=None,
          **changes):
    """the entry point on host arrays with one thing wrong -> (return code, message)"""
    p = _abi.make_channel_params(W, delay=2)
    for k, v in changes.items():
        setattr(p, k, v)
    for name, c, v in cols or ():
        getattr(p, name)[c] = v
    arr = {k: np.zeros((B, W)) for k in ("in0", "in1", "out0", "out1", "dy")}
    st_arr = dict(counter=np.zeros(B, np.int32), ring=np.zeros((3, B, W)), prev=np.zeros((B, W)), d_f=np.zeros((B, W)))
    st = _abi.ChannelState()
    for k, a in st_arr.items():
        setattr(st, k, None if k in state_null else a.ctypes.data)
    g = lambda k: None if k in null else arr[k].ctypes.data
    rc = lib().abrk_channel_step_batch(dtype, C.byref(p) if params else None, B_, g("in0"), w0, g("in1"), w1, g("out0"),
                                       g("out1"), g("dy") if dy else None, C.byref(st) if state else None, 0, None)
    return rc, lib().abrk_last_error().decode()


NAN, INF = float("nan"), float("inf")
EINVAL_CASES = {
    "dtype": dict(dtype=2),
    "negative batch": dict(B_=-1),
    "no width": dict(width=0, w0=0),
    "too wide": dict(width=_abi.CHANNEL_MAX_WIDTH + 1, w0=_abi.CHANNEL_MAX_WIDTH + 1),
    "negative delay": dict(delay=-1),
    "too long a delay": dict(delay=_abi.CHANNEL_MAX_DELAY + 1),
    "widths do not add up": dict(w0=W - 1, w1=0),
    "widths exceed the width": dict(w0=W, w1=1),
    "w1 without in1": dict(w0=W - 1, w1=1, null=("in1",)),
    "w1 without out1": dict(w0=W - 1, w1=1, null=("out1",)),
    "negative sigma": dict(cols=[("sigma", 1, -0.1)]),
    "sigma nan": dict(cols=[("sigma", W - 1, NAN)]),
    "sigma inf": dict(cols=[("sigma", 0, INF)]),
    "negative resolution": dict(cols=[("resolution", 2, -1e-3)]),
    "resolution nan": dict(cols=[("resolution", 0, NAN)]),
    "resolution inf": dict(cols=[("resolution", 0, INF)]),
    "bias nan": dict(cols=[("bias", 3, NAN)]),
    "bias inf": dict(cols=[("bias", 0, -INF)]),
    "dt zero": dict(dt=0.0),
    "dt negative": dict(dt=-1e-3),
    "dt nan": dict(dt=NAN),
    "negative tau_diff with dy": dict(tau_diff=-1.0, dy=True),
    "tau_diff nan with dy": dict(tau_diff=NAN, dy=True),
    "tau_diff inf with dy": dict(tau_diff=INF, dy=True),
    "params": dict(params=False),
    "state": dict(state=False),
    "in0 is NULL": dict(null=("in0",)),
    "out0 is NULL": dict(null=("out0",)),
    "counter is NULL": dict(state_null=("counter",)),
    "ring is NULL with a delay": dict(state_null=("ring",)),
    "prev is NULL with dy": dict(state_null=("prev",), dy=True),
    "d_f is NULL with dy": dict(state_null=("d_f",), dy=True),
}


@pytest.mark.parametrize("what", list(EINVAL_CASES))
def test_einval(what):
    rc, msg = _call(**EINVAL_CASES[what])
    assert rc == -1 and msg, (rc, msg)


def test_an_empty_batch_and_optional_arrays_pass_the_checks():
    # B == 0 returns before the device is touched: what is optional is accepted
    assert _call(B_=0)[0] == 0
    assert _call(B_=0, null=("in1", "out1"))[0] == 0
    assert _call(B_=0, w0=W - 1, w1=1)[0] == 0
    assert _call(B_=0, delay=0, state_null=("ring", "prev", "d_f"))[0] == 0
    assert _call(B_=0, state_null=("prev", "d_f"))[0] == 0
    assert _call(B_=0, dy=True)[0] == 0
    assert _call(B_=0, tau_diff=-1.0)[0] == 0  # tau_diff is only read with dy
    assert _call(B_=0, cols=[("sigma", W, -1.0), ("bias", W, NAN)])[0] == 0  # columns past the width are not read
    e = np.zeros((0, W))
    out = sensing.channel_step(_abi.make_channel_params(W), e, {"counter": np.zeros(0, np.int32)})
    assert out.shape == (0, W)


def test_make_channel_params_broadcasts_and_refuses():
    p = _abi.make_channel_params(3, bias=0.5, sigma=[0.1, 0.0, 0.2], resolution=1e-3, delay=2, seed=(1 << 64) - 1,
                                 row_offset=-7, dt=2e-3, tau_diff=0.01)
    assert (p.width, p.delay, p.seed, p.row_offset, p.dt, p.tau_diff) == (3, 2, (1 << 64) - 1, -7, 2e-3, 0.01)
    assert list(p.bias)[:4] == [0.5, 0.5, 0.5, 0.0] and list(p.sigma)[:3] == [0.1, 0.0, 0.2]
    assert list(p.resolution)[:4] == [1e-3, 1e-3, 1e-3, 0.0]
    for bad in (dict(width=0), dict(width=17), dict(width=3, sigma=[0.1, 0.2]), dict(width=3, bias=np.zeros((3, 1))),
                dict(width=3, seed=-1), dict(width=3, seed=1 << 64)):
        with pytest.raises(ValueError):
            _abi.make_channel_params(**bad)


def test_constructor_arguments():
    got = [(k, p.default) for k, p in inspect.signature(sensing.SignalChannel.__init__).parameters.items() if k != "self"]
    assert got == [("width", inspect.Parameter.empty), ("B", inspect.Parameter.empty), ("bias", 0), ("noise_std", 0),
                   ("resolution", 0), ("delay", 0), ("difference", False), ("tau_diff", 0), ("dt", 0.001), ("seed", 0),
                   ("row_offset", 0), ("dtype", np.float64), ("device", 0), ("stream", None)]
    got = [(k, p.default) for k, p in inspect.signature(sensing.JointSensor.__init__).parameters.items() if k != "self"]
    assert got == [("rc", inspect.Parameter.empty), ("B", inspect.Parameter.empty), ("resolution", 0), ("noise_std", 0),
                   ("bias", 0), ("delay", 0), ("velocity", "measured"), ("noise_std_velocity", 0), ("tau_velocity", 0),
                   ("dt", 0.001), ("seed", 0), ("stream", None)]
    got = list(inspect.signature(sensing.channel_step).parameters)
    assert got == ["params", "in0", "state", "in1", "out0", "out1", "dy", "dtype", "device", "stream"]


@pytest.mark.parametrize("bad", [
    dict(width=0), dict(width=17), dict(B=0), dict(delay=-1), dict(delay=4097), dict(noise_std=-0.1),
    dict(noise_std=NAN), dict(resolution=-1.0), dict(resolution=INF), dict(bias=NAN), dict(dt=0.0), dict(dt=NAN),
    dict(difference=True, tau_diff=-1.0), dict(difference=True, tau_diff=NAN), dict(noise_std=[0.1, 0.2]),
    dict(seed=-1)])
def test_signal_channel_refuses_before_it_allocates(bad):
    kw = dict(width=4, B=8)
    kw.update(bad)
    with pytest.raises(ValueError):
        sensing.SignalChannel(**kw)
    with pytest.raises(TypeError):
        sensing.SignalChannel(4, 8, dtype=np.float16)


def test_joint_sensor_refuses_before_it_allocates():
    from abr_control_amd.arms import ur5

    rc = ur5.Config()
    for bad in (dict(velocity="filtered"), dict(velocity="difference", noise_std_velocity=0.1),
                dict(velocity="measured", tau_velocity=0.01), dict(resolution=[1e-3] * 5), dict(noise_std=-1.0),
                dict(delay=5000), dict(B=0)):
        kw = dict(B=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            sensing.JointSensor(rc, **kw)
