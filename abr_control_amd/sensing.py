"""Measurement and actuation channels of a device-resident control loop: what the law reads is not the plant's exact,
current, continuous state, and what the plant receives is not the law's torque of the same tick.

One kernel (abrk_channel_step_batch, include/abrk.h) passes a [B, W] signal through bias, Gaussian noise, quantisation,
a latency of whole ticks and, optionally, a low-passed difference - one tick per launch, all state in device memory, so it
is recordable into an engine.Plan and launch_graph(K) advances it K times without the host:

    sensor = JointSensor(rc, B, resolution=2 * np.pi / 2**14, delay=2, velocity="difference", tau_velocity=0.005, stream=s)
    actuator = SignalChannel(n, B, delay=1, dtype=rc.dtype, stream=s)
    with engine.Plan(0, s) as tick:
        q_meas, dq_meas = sensor.measure(q, dq)
        engine.osc_generate(rc.arm_id, n, law, q_meas, dq_meas, target, u=u, stream=s)
        u_act = actuator.apply(u)
        engine.plant_step(rc.arm_id, n, plant, q, dq, u_act, stream=s)
    tick.launch_graph(1000)

The noise of (seed, global row, tick, column) is a pure function of those four (Philox4x32-10, Box-Muller in fp64): a
row's bits do not depend on the batch it arrives in, and fp32 sees the realisation fp64 sees.
"""
import ctypes as C

import numpy as np

from . import _abi, engine
from ._lib import DeviceArray, check, lib

CHANNEL_STATE = ("counter", "ring", "prev", "d_f")


def channel_state_shapes(params, B):
    """{name: shape} of the state of channel_step for B rows: counter is int32, the others of the call's dtype; ring is
    needed with delay > 0, prev and d_f with dy"""
    W, d = int(params.width), int(params.delay)
    return {"counter": (B,), "ring": (d + 1, B, W), "prev": (B, W), "d_f": (B, W)}


def channel_step(params, in0, state, in1=None, out0=None, out1=None, dy=None, dtype=np.float64, device=0, stream=None):
    """One tick of the channel (abrk_channel_step_batch) - recordable into a Plan.  params: _abi.make_channel_params.  The
    row's input is concat(in0[b], in1[b]) ([B,w0], [B,w1] with w0 + w1 = params.width); state: a dict of the arrays of
    channel_state_shapes (ring may be missing with delay 0, prev and d_f without dy), updated in place.  out0 / out1:
    preallocated outputs, mirroring the inputs; dy: True or a [B,width] array for the filtered difference of the output.
    -> out0, or a tuple (out0[, out1][, dy]).  All arrays are of `dtype`, NumPy or DeviceArray alike."""
    a = engine._Args(dtype, device)
    W = int(params.width)
    B, w0 = in0.shape[0], in0.shape[1]
    w1 = 0 if in1 is None else in1.shape[1]
    i0p, i1p = a.inp(in0, (B, w0), "in0"), a.inp(in1, (B, w1), "in1")
    st = _abi.ChannelState()
    shapes = channel_state_shapes(params, B)
    counter = state.get("counter")
    if counter is not None:
        st.counter = a.side(counter, shapes["counter"], "counter")
    for name in ("ring", "prev", "d_f"):
        arr = state.get(name)
        if arr is not None:
            setattr(st, name, a.inout(arr, shapes[name], name))
    o0p, o0 = a.out(out0, (B, w0), "out0")
    o1p, o1 = a.out(out1, (B, w1), "out1") if in1 is not None else (None, None)
    dyp, dyo = a.opt_out(dy, (B, W), "dy")
    check(lib().abrk_channel_step_batch(a.code, C.byref(params), B, i0p, w0, i1p, w1, o0p, o1p, dyp, C.byref(st), device,
                                        engine._sp(stream)))
    ret = tuple(x for x in (o0, o1, dyo) if x is not None)
    return ret[0] if len(ret) == 1 else ret


class SignalChannel:
    """A channel of `width` columns for B rows that owns its state - tick counter, delay ring, the differencer's two
    arrays - and its output buffers, as LoopRecorder owns its buffers.

    bias, noise_std, resolution: scalars, or one value per column; delay: whole ticks (for the first `delay` ticks after
    a reset the channel holds its first sample); difference: also return d/dt of the output, low-passed with tau_diff
    (0: the plain difference quotient; 0 at the first tick); seed, row_offset: the noise of row b is that of global row
    b + row_offset under `seed`; stream: the stream apply() and reset() run on."""

    def __init__(self, width, B, bias=0, noise_std=0, resolution=0, delay=0, difference=False, tau_diff=0, dt=0.001,
                 seed=0, row_offset=0, dtype=np.float64, device=0, stream=None):
        B, delay = int(B), int(delay)
        if B < 1:
            raise ValueError(f"B={B} < 1")
        if not 0 <= delay <= _abi.CHANNEL_MAX_DELAY:
            raise ValueError(f"delay={delay} outside 0..{_abi.CHANNEL_MAX_DELAY}")
        self.params = _abi.make_channel_params(width, bias, noise_std, resolution, delay, seed, row_offset, dt, tau_diff)
        W = self.width = int(self.params.width)
        for name in ("sigma", "resolution", "bias"):
            col = np.array(getattr(self.params, name)[:W])
            if not np.isfinite(col).all() or (name != "bias" and (col < 0).any()):
                raise ValueError(f"{'noise_std' if name == 'sigma' else name}: finite"
                                 f"{'' if name == 'bias' else ' and not negative'}, got {col}")
        if not (np.isfinite(self.params.dt) and self.params.dt > 0):
            raise ValueError(f"dt={dt} is not a positive finite step")
        if difference and not (np.isfinite(self.params.tau_diff) and self.params.tau_diff >= 0):
            raise ValueError(f"tau_diff={tau_diff} is negative or not finite")
        self.B, self.delay, self.difference = B, delay, bool(difference)
        self.dtype, self.device, self.stream = engine._dtype_of(dtype)[0], device, stream
        mk = lambda shape: DeviceArray(shape, self.dtype, device)
        self._state = {"counter": DeviceArray((B,), np.int32, device)}
        if delay:
            self._state["ring"] = mk((delay + 1, B, W))
        if self.difference:
            self._state["prev"], self._state["d_f"] = mk((B, W)), mk((B, W))
        self._dy = mk((B, W)) if self.difference else None
        self._out = None  # allocated by the first apply(), which fixes how the columns are split
        self.reset()

    def apply(self, x, x1=None):
        """One tick (inside `with engine.Plan(...)`: recorded).  x [B,w0] and, when the columns come from two arrays,
        x1 [B,w1], w0 + w1 = width: DeviceArrays of the channel's dtype.  -> the channel's own output DeviceArray, or a
        tuple (y[, y1][, dy]); the same arrays at every call."""
        split = (x.shape[1], 0 if x1 is None else x1.shape[1])
        if x.shape[0] != self.B or sum(split) != self.width:
            raise ValueError(f"this channel passes {self.B} rows of {self.width} columns; got {x.shape}"
                             + ("" if x1 is None else f" and {x1.shape}"))
        if self._out is None:
            self._out = (split, DeviceArray((self.B, split[0]), self.dtype, self.device),
                         None if x1 is None else DeviceArray((self.B, split[1]), self.dtype, self.device))
        elif self._out[0] != split:
            raise ValueError(f"this channel's columns are split {self._out[0]}; got {split}")
        return channel_step(self.params, x, self._state, in1=x1, out0=self._out[1], out1=self._out[2], dy=self._dy,
                            dtype=self.dtype, device=self.device, stream=self.stream)

    def reset(self, rows=None):
        """Restart all rows, or rows [lo, hi): a zero fill of their tick counter on the channel's stream (ordered with
        the ticks enqueued there before and after it).  Nothing else needs clearing."""
        lo, hi = (0, self.B) if rows is None else (int(rows[0]), int(rows[1]))
        self._state["counter"].rows(lo, hi).zero_(self.stream)

    def ticks(self):
        """the tick counter of every row, [B]"""
        return self._state["counter"].numpy(self.stream).astype(np.int64)

    def device_state(self):
        """{"counter": int32 [B], "ring": [delay + 1, B, W], "prev": [B, W], "d_f": [B, W]} - those the channel has"""
        return dict(self._state)


class JointSensor:
    """What a law reads of the n joints of the arm `rc` (a robot_config of this package) for B rows: encoders with a
    `resolution` (rad per count), noise of standard deviation `noise_std`, a `bias` and a latency of `delay` ticks.

    velocity="measured": q and dq go through one channel of width 2n - the velocity columns carry the same latency,
    noise of standard deviation noise_std_velocity and neither bias nor quantisation.  velocity="difference": q alone
    goes through the channel, and dq_meas is the difference of consecutive position measurements over dt, low-passed with
    tau_velocity (0: the plain difference quotient) - the dq argument of measure() is then not read."""

    def __init__(self, rc, B, resolution=0, noise_std=0, bias=0, delay=0, velocity="measured", noise_std_velocity=0,
                 tau_velocity=0, dt=0.001, seed=0, stream=None):
        if velocity not in ("measured", "difference"):
            raise ValueError(f"velocity={velocity!r}: 'measured' or 'difference'")
        n = self.n = rc.N_JOINTS
        self.velocity = velocity
        col = lambda v, name: _joint_column(v, n, name)
        kw = dict(delay=delay, dt=dt, seed=seed, dtype=rc.dtype, device=rc.device, stream=stream)
        if velocity == "measured":
            if 2 * n > _abi.CHANNEL_MAX_WIDTH:
                raise ValueError(f"velocity='measured' passes 2 n = {2 * n} columns; a channel has at most "
                                 f"{_abi.CHANNEL_MAX_WIDTH}: use velocity='difference'")
            if tau_velocity:
                raise ValueError("tau_velocity filters the differenced velocity: velocity='difference'")
            zeros = np.zeros(n)
            self.channel = SignalChannel(
                2 * n, B, bias=np.concatenate([col(bias, "bias"), zeros]),
                noise_std=np.concatenate([col(noise_std, "noise_std"), col(noise_std_velocity, "noise_std_velocity")]),
                resolution=np.concatenate([col(resolution, "resolution"), zeros]), **kw)
        else:
            if np.any(np.asarray(noise_std_velocity) != 0):
                raise ValueError("noise_std_velocity belongs to a measured velocity: velocity='measured'")
            self.channel = SignalChannel(n, B, bias=col(bias, "bias"), noise_std=col(noise_std, "noise_std"),
                                         resolution=col(resolution, "resolution"), difference=True,
                                         tau_diff=tau_velocity, **kw)

    def measure(self, q, dq=None):
        """One tick in one launch (inside `with engine.Plan(...)`: recorded): DeviceArrays q, dq [B,n] -> (q_meas,
        dq_meas), the sensor's own arrays."""
        if self.velocity == "measured":
            if dq is None:
                raise ValueError("velocity='measured' needs dq")
            return self.channel.apply(q, dq)
        return self.channel.apply(q)

    def reset(self, rows=None):
        self.channel.reset(rows)


def _joint_column(v, n, name):
    col = np.asarray(v, dtype=float)
    if col.ndim > 1 or (col.ndim == 1 and col.shape[0] != n):
        raise ValueError(f"{name}: a scalar or one value per joint ({n}), got shape {col.shape}")
    return np.broadcast_to(col, (n,)).copy()
