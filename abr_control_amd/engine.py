"""Batched calls into libabrk.so.

Every function takes either NumPy arrays (staged through device scratch by the library,
results returned as NumPy) or `DeviceArray`s (zero-copy, asynchronous on `stream`, results
returned as `DeviceArray`s).  Shapes are `[B, ...]`, row-major; dtype float64 or float32
selects the arithmetic of the kernels.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._lib import NP_DTYPE, AbrkError, DeviceArray, check, lib  # noqa: F401
from .sharding import ShardedArray

_OUT_SHAPES = {
    "Tx": lambda n: (3,),
    "J": lambda n: (6, n),
    "M": lambda n: (n, n),
    "g": lambda n: (n,),
    "C": lambda n: (n, n),
    "dJ": lambda n: (6, n),
    "R": lambda n: (3, 3),
    "T": lambda n: (4, 4),
    "Tinv": lambda n: (4, 4),
    "quat": lambda n: (4,),
}
_WANT_BITS = {
    "Tx": _abi.WANT_TX, "J": _abi.WANT_J, "M": _abi.WANT_M, "g": _abi.WANT_G, "C": _abi.WANT_C,
    "dJ": _abi.WANT_DJ, "R": _abi.WANT_R, "T": _abi.WANT_T, "Tinv": _abi.WANT_TINV, "quat": _abi.WANT_QUAT,
}


def _dtype_code(dtype):
    dt = np.dtype(dtype)
    if dt == np.float64:
        return _abi.F64
    if dt == np.float32:
        return _abi.F32
    raise TypeError(f"abr_control_amd computes in float64 or float32, not {dt}")


# (np.dtype, ABRK_F64 / ABRK_F32) of the spellings callers use, looked up once per call; any other goes the long way
_DTYPES = {k: (np.dtype(k), _dtype_code(k)) for t in (np.float64, np.float32) for k in (t, np.dtype(t))}


def _dtype_of(dtype):
    return _DTYPES.get(dtype) or (np.dtype(dtype), _dtype_code(dtype))


def _sp(stream):
    return None if stream is None else getattr(stream, "ptr", stream)


class _Marshal:
    """What every marshaller of array arguments offers, wherever the call runs (one device: _Args; one host batch over
    several devices: _HostBatch; shards resident on devices: _Cut).  inp / out / inout / side bind an input, an output
    (-> pointer, object to return), a state array updated in place and an int32 or float64 side array; shapes are the
    whole batch's, [B, ...], as tuples.  `form` names the C entry (abrk_<family>_<form>), `batch(B)` is what that entry
    takes for the batch (the row count, or the cut) and `where` its trailing arguments."""

    def opt_out(self, flag, shape, name):
        """an output the caller may leave out: False / None (-> None, None), True (allocated here) or the array"""
        if flag is None or flag is False:
            return None, None
        return self.out(None if flag is True else flag, shape, name)

    def want(self, names, n, B, out=None, offered=None):
        """the robot_config outputs `names` -> (ABRK_WANT_* bits, the abrk_dyn_out argument, {name: array}); `out`: a
        dict of preallocated arrays"""
        bits, ptrs, res = 0, {}, {}
        for name in names:
            if offered is not None and name not in offered:
                raise ValueError(f"the fused kernel offers {', '.join(offered)} - not {name!r}")
            bits |= _WANT_BITS[name]
            ptrs[name], res[name] = self.out(None if out is None else out.get(name), (B,) + _OUT_SHAPES[name](n), name)
        return bits, self._dyn_out(ptrs), res


class _Args(_Marshal):
    """One device: NumPy arrays (staged by the library; host copies are kept alive here) or DeviceArrays, not both."""
    form = "batch"
    on_device = None  # decided by the first array
    mixed = "mixing DeviceArray and NumPy arguments in one call is not supported"

    def __init__(self, dtype, device=0, stream=None):
        self.np_dtype, self.code = _dtype_of(dtype)
        self.keep = []
        self.device = device
        self.where = (device, _sp(stream))

    def batch(self, B):
        return B

    def _mode(self, dev, name):
        if self.on_device is None:
            self.on_device = dev
        elif self.on_device != dev:
            raise TypeError(f"{name}: {self.mixed}")

    def inp(self, a, shape, name):
        if a is None:
            return None
        if isinstance(a, DeviceArray):
            if self.on_device is not True:
                self._mode(True, name)
            if a.dtype != self.np_dtype or a.shape != shape:
                raise ValueError(f"{name}: expected {self.np_dtype}{shape}, got {a.dtype}{a.shape}")
            return a.ptr
        if self.on_device is not False:
            self._mode(False, name)
        h = np.ascontiguousarray(a, dtype=self.np_dtype)
        if h.shape != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {h.shape}")
        self.keep.append(h)
        return h.ctypes.data

    def out(self, given, shape, name):
        if self.on_device:
            if given is None:
                given = DeviceArray(shape, self.np_dtype, self.device)
            elif not isinstance(given, DeviceArray) or given.shape != shape or given.dtype != self.np_dtype:
                raise ValueError(f"{name}: output must be a DeviceArray {self.np_dtype}{shape}")
            return given.ptr, given
        if given is None:
            given = np.empty(shape, self.np_dtype)
        elif (not isinstance(given, np.ndarray) or given.shape != shape or given.dtype != self.np_dtype
              or not given.flags.c_contiguous):
            raise ValueError(f"{name}: output must be a C-contiguous ndarray {self.np_dtype}{shape}")
        return given.ctypes.data, given

    def inout(self, arr, shape, name):
        """a DeviceArray, or a C-contiguous ndarray of the call dtype: it is written, so no copy may stand in for it"""
        if arr is None:
            return None
        if isinstance(arr, DeviceArray):
            return self.inp(arr, shape, name)
        if (not isinstance(arr, np.ndarray) or arr.dtype != self.np_dtype or arr.shape != shape
                or not arr.flags.c_contiguous):
            raise ValueError(f"{name} must be a C-contiguous ndarray {shape} of the call dtype (updated in place)")
        self._mode(False, name)
        return arr.ctypes.data

    def side(self, arr, shape, name, dtype=np.int32):
        """an array of a dtype of its own (int32 counters, float64 statistics), passed as it is"""
        dev = isinstance(arr, DeviceArray)
        self._mode(dev, name)
        if arr.dtype != dtype or tuple(arr.shape) != shape or (not dev and not arr.flags.c_contiguous):
            raise ValueError(f"{name}: expected a C-contiguous {np.dtype(dtype)} array {shape}, "
                             f"got {arr.dtype}{tuple(arr.shape)}")
        return arr.ptr if dev else arr.ctypes.data

    def _dyn_out(self, ptrs):
        return C.byref(_abi.DynOut(**ptrs))


class _HostBatch(_Args):
    """ONE host batch cut into contiguous row shards, shard g on devices[g]: NumPy arrays only."""
    form = "sharded"
    on_device = False
    mixed = "the sharded calls take NumPy arrays (a DeviceArray lives on one device)"

    def __init__(self, dtype, devices):
        _Args.__init__(self, dtype)
        self.where = (len(devices), (C.c_int * len(devices))(*[int(d) for d in devices]))

    def out(self, given, shape, name):
        self._mode(isinstance(given, DeviceArray), name)
        return _Args.out(self, given, shape, name)

    def inout(self, arr, shape, name):
        self._mode(isinstance(arr, DeviceArray), name)
        return _Args.inout(self, arr, shape, name)


class _PlanArgs(_Args):
    """The fixed buffers of a launch plan: DeviceArrays only, the outputs too."""
    on_device = True
    mixed = "launch plans take DeviceArrays"

    def out(self, given, shape, name):
        self._mode(isinstance(given, DeviceArray), name)
        return _Args.out(self, given, shape, name)

    inout = _Args.inp


class _Cut(_Marshal):
    """Shards resident on devices: abrk_shard_cut + the per-shard pointer tables of one call, whose arrays
    are sharding.ShardedArrays cut like `like`; shard g runs on streams[g], or on the library's own stream of its
    (device, slot)."""
    form, where = "resident", ()

    def __init__(self, like, dtype, streams=None):
        self.devices, self.rows = list(like.devices), list(like.rows)
        self.G = len(self.devices)
        self.np_dtype, self.code = _dtype_of(dtype)
        self._dev = (C.c_int32 * self.G)(*self.devices)
        self._rows = (C.c_int64 * self.G)(*self.rows)
        self._streams = None
        if streams is not None:
            if len(streams) != self.G:
                raise ValueError(f"{len(streams)} streams for {self.G} shards")
            self._streams = (C.c_void_p * self.G)(*[_sp(st) for st in streams])
        self.c = _abi.ShardCut(self.G, self._dev, self._rows, self._streams)

    def batch(self, B):
        return C.byref(self.c)

    def inp(self, arr, shape, name, dtype=None):
        """pointer table of a ShardedArray (None -> NULL), checked against the cut"""
        if arr is None:
            return None
        if list(arr.devices) != self.devices or list(arr.rows) != self.rows:
            raise ValueError(f"{name}: cut over other devices / rows than q")
        if arr.dtype != (dtype or self.np_dtype) or tuple(arr.shape) != tuple(shape):
            raise ValueError(f"{name}: expected {np.dtype(dtype or self.np_dtype)}{tuple(shape)}, got {arr.dtype}{arr.shape}")
        return (C.c_void_p * self.G)(*[p.ptr for p in arr.parts])

    inout = inp

    def side(self, arr, shape, name, dtype=np.int32):
        return self.inp(arr, shape, name, dtype)

    def out(self, given, shape, name):
        if given is None:
            given = ShardedArray.empty(shape, self.np_dtype, self.devices, rows=self.rows)
        return self.inp(given, shape, name), given

    def _dyn_out(self, tables):
        dos = (_abi.DynOut * self.G)()
        for name, table in tables.items():
            for do, ptr in zip(dos, table):
                setattr(do, name, ptr)
        return dos


def _marshaller(where, dtype, q):
    """where a controller's call runs -> its marshaller.  where: a device ordinal; a list of device ordinals that one
    host batch is cut over; or, when q is a ShardedArray, the streams of its shards (None: the library's own)"""
    if isinstance(q, ShardedArray):
        return _Cut(q, dtype, where)
    return _HostBatch(dtype, where) if isinstance(where, list) else _Args(dtype, where)


# ---------------------------------------------------------------------------- the four families with sharded forms
# One binder each: the family's arrays, their row shapes and roles, stated once against whichever marshaller `m` the
# call runs on.  The C entries of a family take the same arguments but for m.batch / m.where.
def _entry(family, m):
    return getattr(lib(), f"abrk_{family}_{m.form}")


def _bind_osc(m, n, q, dq, target, target_velocity, integrated_error, u_null_ext, u, training_signal):
    """-> (B, the eight array arguments of the abrk_osc_* entries, u or (u, training_signal))"""
    B = q.shape[0]
    joints, task = (B, n), (B, 6)
    inp = m.inp
    ptrs = [inp(q, joints, "q"), inp(dq, joints, "dq"), inp(target, task, "target"),
            inp(target_velocity, task, "target_velocity"), m.inout(integrated_error, task, "integrated_error"),
            inp(u_null_ext, joints, "u_null_ext"), None, None]
    ptrs[6], uo = m.out(u, joints, "u")
    ptrs[7], tso = m.opt_out(training_signal, joints, "training_signal")
    return B, ptrs, uo if tso is None else (uo, tso)


def _osc(m, arm_id, n, params, q, dq, target, target_velocity=None, integrated_error=None, u_null_ext=None, u=None,
         training_signal=False):
    B, ptrs, ret = _bind_osc(m, n, q, dq, target, target_velocity, integrated_error, u_null_ext, u, training_signal)
    check(_entry("osc_generate", m)(arm_id, m.code, C.byref(params), m.batch(B), *ptrs, *m.where))
    return ret


def _bind_sliding(m, n, params, q, dq, target, target_velocity, target_acc, u, want_s):
    """-> (B, the seven array arguments of the abrk_sliding_* entries, u or (u, s))"""
    B = q.shape[0]
    nt = 3 if params.cartesian else n
    ptrs = [m.inp(q, (B, n), "q"), m.inp(dq, (B, n), "dq"), m.inp(target, (B, nt), "target"),
            m.inp(target_velocity, (B, nt), "target_velocity"), m.inp(target_acc, (B, nt), "target_acc")]
    up, uo = m.out(u, (B, n), "u")
    sp, so = m.opt_out(want_s, (B, n), "s")
    return B, ptrs + [up, sp], uo if so is None else (uo, so)


def _sliding(m, arm_id, n, params, q, dq, target, target_velocity=None, target_acc=None, u=None, want_s=False):
    B, ptrs, ret = _bind_sliding(m, n, params, q, dq, target, target_velocity, target_acc, u, want_s)
    check(_entry("sliding_generate", m)(arm_id, m.code, C.byref(params), m.batch(B), *ptrs, *m.where))
    return ret


def _joint(m, arm_id, n, ctrl, account_for_gravity, q, dq, target=None, target_velocity=None, u=None):
    B = q.shape[0]
    ptrs = [m.inp(q, (B, n), "q"), m.inp(dq, (B, n), "dq"), m.inp(target, (B, n), "target"),
            m.inp(target_velocity, (B, n), "target_velocity")]
    up, uo = m.out(u, (B, n), "u")
    check(_entry("joint_generate", m)(arm_id, m.code, C.byref(ctrl), int(bool(account_for_gravity)), m.batch(B), *ptrs, up,
                                      *m.where))
    return uo


def _dynamics(m, arm_id, n, q, dq, frame, x_off, want, out=None):
    B = q.shape[0]
    frame = 2 * n + 1 if frame is None else frame
    qp, dqp = m.inp(q, (B, n), "q"), m.inp(dq, (B, n), "dq")
    bits, do, res = m.want(want, n, B, out)
    xo = None if x_off is None else (C.c_double * 3)(*[float(v) for v in x_off])
    check(_entry("dynamics", m)(arm_id, m.code, m.batch(B), qp, dqp, frame, xo, bits, do, *m.where))
    return res


def dynamics(arm_id, n, q, dq=None, frame=None, x_off=None, want=("M",), dtype=np.float64, device=0,
             stream=None, out=None):
    """robot_config.{Tx,J,M,g,C,dJ,R,T,T_inv,quaternion} for a batch (one launch, shared FK).
    Returns {name: array[B, ...]} for every name in `want`."""
    return _dynamics(_Args(dtype, device, stream), arm_id, n, q, dq, frame, x_off, want, out)


def osc_generate(arm_id, n, params, q, dq, target, target_velocity=None, integrated_error=None,
                 u_null_ext=None, u=None, training_signal=False, dtype=np.float64, device=0, stream=None,
                 want=None, out=None):
    """OSC.generate for a batch.  `integrated_error` ([B,6]) is updated in place when ki != 0.
    Returns u, or (u, training_signal) when training_signal is True / an output array.
    want: subset of ("Tx", "J", "M", "g", "C", "dJ") -> the fused kernel (abrk_osc_generate_full_batch) also writes those
    robot_config outputs of the controller's ref_frame / xyz_offset; the return value gains a dict of them
    (`out`: optional dict of preallocated arrays)."""
    m = _Args(dtype, device, stream)
    B, ptrs, ret = _bind_osc(m, n, q, dq, target, target_velocity, integrated_error, u_null_ext, u, training_signal)
    if not want:  # (the call a host-driven loop makes per tick: its entry is named here, not looked up as _osc does)
        check(lib().abrk_osc_generate_batch(arm_id, m.code, C.byref(params), B, *ptrs, *m.where))
        return ret
    bits, do, res = m.want(want, n, B, out, ("Tx", "J", "M", "g", "C", "dJ"))
    check(lib().abrk_osc_generate_full_batch(arm_id, m.code, C.byref(params), B, *ptrs, bits, do, *m.where))
    return ret + (res,) if type(ret) is tuple else (ret, res)


def osc_generate_coop(arm_id, n, params, q, dq, target, lanes_per_arm, u=None, training_signal=False, dtype=np.float64,
                      device=0, stream=None):
    """The wave-cooperative mapping of the plain OSC law (abrk_osc_generate_coop_batch; ur5, fp64): K = lanes_per_arm
    lanes per arm instance.  Measurement variant - see profiles/round2/coop_ab.md."""
    a = _Args(dtype, device)
    B = q.shape[0]
    qp = a.inp(q, (B, n), "q")
    dqp = a.inp(dq, (B, n), "dq")
    tp = a.inp(target, (B, 6), "target")
    up, uo = a.out(u, (B, n), "u")
    tsp, tso = a.opt_out(training_signal, (B, n), "training_signal")
    check(lib().abrk_osc_generate_coop_batch(arm_id, a.code, C.byref(params), B, qp, dqp, tp, up, tsp,
                                             int(lanes_per_arm), device, _sp(stream)))
    return (uo, tso) if tso is not None else uo


def osc_generate_sharded(arm_id, n, params, q, dq, target, devices, target_velocity=None, integrated_error=None,
                         u_null_ext=None, u=None, training_signal=False, dtype=np.float64):
    """OSC.generate of ONE host batch over several devices (abrk_osc_generate_sharded): contiguous row shards, shard g
    on devices[g], no collective.  NumPy arrays only.  Returns u or (u, training_signal)."""
    return _osc(_HostBatch(dtype, devices), arm_id, n, params, q, dq, target, target_velocity, integrated_error,
                u_null_ext, u, training_signal)


def sliding_generate_sharded(arm_id, n, params, q, dq, target, devices, target_velocity=None, target_acc=None,
                             want_s=False, dtype=np.float64):
    """Sliding.generate of ONE host batch over several devices (abrk_sliding_generate_sharded)"""
    return _sliding(_HostBatch(dtype, devices), arm_id, n, params, q, dq, target, target_velocity, target_acc, None,
                    bool(want_s))


def joint_generate_sharded(arm_id, n, ctrl, account_for_gravity, q, dq, devices, target=None, target_velocity=None,
                           dtype=np.float64):
    """Joint / Damping / RestingConfig.generate of ONE host batch over several devices (abrk_joint_generate_sharded)"""
    return _joint(_HostBatch(dtype, devices), arm_id, n, ctrl, account_for_gravity, q, dq, target, target_velocity)


def dynamics_sharded(arm_id, n, q, devices, dq=None, frame=None, x_off=None, want=("M",), dtype=np.float64):
    """robot_config.{Tx,J,M,g,C,dJ,R,T,T_inv,quaternion} of ONE host batch over several devices (abrk_dynamics_sharded)"""
    return _dynamics(_HostBatch(dtype, devices), arm_id, n, q, dq, frame, x_off, want)


def osc_generate_resident(arm_id, n, params, q, dq, target, target_velocity=None, integrated_error=None,
                          u_null_ext=None, u=None, training_signal=False, dtype=np.float64, streams=None):
    """OSC.generate on a batch whose shards LIVE on the devices (abrk_osc_generate_resident): every array a
    sharding.ShardedArray cut the same way; the call only enqueues (shard g on streams[g], or on the library's own
    stream of its (device, slot)).  integrated_error [B,6] stays with its shards.  Returns u, or (u, training_signal),
    as ShardedArrays - not yet complete: sync with `shards_sync(u)` / MultiDevice.sync()."""
    return _osc(_Cut(q, dtype, streams), arm_id, n, params, q, dq, target, target_velocity, integrated_error, u_null_ext,
                u, training_signal)


def sliding_generate_resident(arm_id, n, params, q, dq, target, target_velocity=None, target_acc=None, u=None,
                              want_s=False, dtype=np.float64, streams=None):
    """Sliding.generate on resident shards (abrk_sliding_generate_resident)"""
    return _sliding(_Cut(q, dtype, streams), arm_id, n, params, q, dq, target, target_velocity, target_acc, u, want_s)


def joint_generate_resident(arm_id, n, ctrl, account_for_gravity, q, dq, target=None, target_velocity=None, u=None,
                            dtype=np.float64, streams=None):
    """Joint / Damping / RestingConfig.generate on resident shards (abrk_joint_generate_resident)"""
    return _joint(_Cut(q, dtype, streams), arm_id, n, ctrl, account_for_gravity, q, dq, target, target_velocity, u)


def dynamics_resident(arm_id, n, q, dq=None, frame=None, x_off=None, want=("M",), dtype=np.float64, streams=None,
                      out=None):
    """robot_config.{Tx,J,M,g,C,dJ,R,T,T_inv,quaternion} on resident shards (abrk_dynamics_resident):
    {name: ShardedArray}"""
    return _dynamics(_Cut(q, dtype, streams), arm_id, n, q, dq, frame, x_off, want, out)


def shards_sync(like, streams=None):
    """drain the streams of a resident batch (abrk_shards_sync): raises SingularMatrixError once if any shard met a
    singular M"""
    c = _Cut(like, like.dtype, streams)
    check(lib().abrk_shards_sync(C.byref(c.c)))


def plans_launch(plans, repeat=1, graph=False):
    """`repeat` ticks of several recorded plans (one per shard / device) from ONE call (abrk_plans_launch)"""
    ids = (C.c_int * len(plans))(*[p.id for p in plans])
    check(lib().abrk_plans_launch(ids, len(plans), int(repeat), 1 if graph else 0))


def osc_law(n, params, J, M, dq, target, g=None, Cdq=None, xyz=None, R=None, q=None, target_velocity=None,
            integrated_error=None, u_null_ext=None, training_signal=False, dtype=np.float64, device=0, stream=None):
    """The OSC control law on caller-supplied dynamics (abrk_osc_law_batch): J [B,6,n], M [B,n,n] and,
    as the controller options require, g [B,n], Cdq [B,n], xyz [B,3], R [B,3,3], q [B,n]."""
    a = _Args(dtype, device)
    B = J.shape[0]
    Jp = a.inp(J, (B, 6, n), "J")
    Mp = a.inp(M, (B, n, n), "M")
    gp = a.inp(g, (B, n), "g")
    cp = a.inp(Cdq, (B, n), "Cdq")
    xp = a.inp(xyz, (B, 3), "xyz")
    Rp = a.inp(R, (B, 3, 3), "R")
    qp = a.inp(q, (B, n), "q")
    dqp = a.inp(dq, (B, n), "dq")
    tp = a.inp(target, (B, 6), "target")
    tvp = a.inp(target_velocity, (B, 6), "target_velocity")
    unp = a.inp(u_null_ext, (B, n), "u_null_ext")
    iep = a.inout(integrated_error, (B, 6), "integrated_error")
    up, uo = a.out(None, (B, n), "u")
    tsp, tso = a.opt_out(bool(training_signal), (B, n), "training_signal")
    check(lib().abrk_osc_law_batch(n, a.code, C.byref(params), B, Jp, Mp, gp, cp, xp, Rp, qp, dqp, tp, tvp, iep, unp,
                                   up, tsp, device, _sp(stream)))
    return (uo, tso) if tso is not None else uo


def osc_mx(n, M, J, threshold=1e-3, want_minv=True, dtype=np.float64, device=0, stream=None):
    """OSC._Mx (osc.py:120-147) for B rows: M [B,n,n], J [B,k,n] -> (Mx [B,k,k], M_inv [B,n,n] or None)"""
    a = _Args(dtype, device)
    B, k = J.shape[0], J.shape[1]
    Mp = a.inp(M, (B, n, n), "M")
    Jp = a.inp(J, (B, k, n), "J")
    xp, xo = a.out(None, (B, k, k), "Mx")
    ip, io = a.out(None, (B, n, n), "M_inv") if want_minv else (None, None)
    check(lib().abrk_osc_mx_batch(n, k, a.code, B, Mp, Jp, float(threshold), xp, ip, device, _sp(stream)))
    return xo, io


def osc_velocity_limiting(params, u_task, dtype=np.float64, device=0, stream=None):
    """OSC._velocity_limiting (osc.py:198-215) for B rows of u_task [B,6]"""
    a = _Args(dtype, device)
    B = u_task.shape[0]
    ip = a.inp(u_task, (B, 6), "u_task")
    op, oo = a.out(None, (B, 6), "out")
    check(lib().abrk_osc_velocity_limiting_batch(a.code, C.byref(params), B, ip, op, device, _sp(stream)))
    return oo


def osc_orientation_forces(algorithm, R, target_abg, dtype=np.float64, device=0, stream=None):
    """OSC._calc_orientation_forces (osc.py:149-196) from R [B,3,3] = robot_config.R(ref_frame, q), target_abg [B,3]"""
    a = _Args(dtype, device)
    B = R.shape[0]
    Rp = a.inp(R, (B, 3, 3), "R")
    tp = a.inp(target_abg, (B, 3), "target_abg")
    op, oo = a.out(None, (B, 3), "u_task_orientation")
    check(lib().abrk_osc_orientation_forces_batch(int(algorithm), a.code, B, Rp, tp, op, device, _sp(stream)))
    return oo


_TF_WIDTHS = {0: (3, 0, 4), 1: (3, 0, 4), 2: (9, 0, 4), 3: (4, 4, 4), 4: (4, 0, 4), 5: (4, 0, 4), 6: (3, 0, 3),
              7: (3, 0, 9)}


def transformations(op, a, b=None, dtype=np.float64, device=0, stream=None):
    """abrk_transformations_batch: op = ABRK_TF_* (include/abrk.h); a [B,wa], b [B,wb] or None -> out [B,wo]"""
    wa, wb, wo = _TF_WIDTHS[int(op)]
    ar = _Args(dtype, device)
    B = a.shape[0]
    ap = ar.inp(a, (B, wa), "a")
    bp = ar.inp(b, (B, wb), "b") if wb else None
    op_, oo = ar.out(None, (B, wo), "out")
    check(lib().abrk_transformations_batch(int(op), ar.code, B, ap, bp, op_, device, _sp(stream)))
    return oo


def sliding_generate(arm_id, n, params, q, dq, target, target_velocity=None, target_acc=None, u=None,
                     want_s=False, dtype=np.float64, device=0, stream=None):
    return _sliding(_Args(dtype, device, stream), arm_id, n, params, q, dq, target, target_velocity, target_acc, u,
                    bool(want_s))


def joint_generate(arm_id, n, ctrl, account_for_gravity, q, dq, target=None, target_velocity=None, u=None,
                   dtype=np.float64, device=0, stream=None):
    return _joint(_Args(dtype, device, stream), arm_id, n, ctrl, account_for_gravity, q, dq, target, target_velocity, u)


def avoid_joint_limits_generate(n, params, q, u=None, accumulate=False, dtype=np.float64, device=0, stream=None):
    """AvoidJointLimits.generate for B states; accumulate: u += signal (u must then be given)."""
    a = _Args(dtype, device)
    B = q.shape[0]
    qp = a.inp(q, (B, n), "q")
    up, uo = a.out(u, (B, n), "u")
    check(lib().abrk_avoid_joint_limits_generate_batch(n, a.code, C.byref(params), B, qp, up,
                                                       int(bool(accumulate and u is not None)), device, _sp(stream)))
    return uo


def floating_generate(arm_id, n, dynamic, task_space, q, dq=None, u=None, accumulate=False, dtype=np.float64,
                      device=0, stream=None):
    """Floating.generate for B states."""
    a = _Args(dtype, device)
    B = q.shape[0]
    qp = a.inp(q, (B, n), "q")
    dqp = a.inp(dq, (B, n), "dq") if dynamic else None
    up, uo = a.out(u, (B, n), "u")
    check(lib().abrk_floating_generate_batch(arm_id, a.code, int(bool(dynamic)), int(bool(task_space)), B, qp, dqp,
                                             up, int(bool(accumulate and u is not None)), device, _sp(stream)))
    return uo


def avoid_obstacles_generate(arm_id, n, params, q, u=None, accumulate=False, dtype=np.float64, device=0,
                             stream=None):
    """AvoidObstacles.generate for B states (obstacles shared by all rows)."""
    a = _Args(dtype, device)
    B = q.shape[0]
    qp = a.inp(q, (B, n), "q")
    up, uo = a.out(u, (B, n), "u")
    check(lib().abrk_avoid_obstacles_generate_batch(arm_id, a.code, C.byref(params), B, qp, up,
                                                    int(bool(accumulate and u is not None)), device, _sp(stream)))
    return uo


def twolink_step(plant, q, dq, u, dtype=np.float64, device=0, stream=None):
    """ArmSim._step for a batch: (q, dq) [B,2] advanced in place by torques u [B,2]."""
    a = _Args(dtype, device)
    B = q.shape[0]
    qp, dqp = a.inout(q, (B, 2), "q"), a.inout(dq, (B, 2), "dq")
    up = a.inp(u, (B, 2), "u")
    check(lib().abrk_twolink_step_batch(a.code, C.byref(plant), B, qp, dqp, up, device, _sp(stream)))


def forward_dynamics(arm_id, n, q, dq, u, ddq=None, dtype=np.float64, device=0, stream=None, effects=None,
                     tau_ext=None, wrench=None):
    """ddq = M(q)^-1 (tau - C(q,dq) dq - g(q)) for B states: q, dq, u [B,n] -> ddq [B,n].  tau = u, or with `effects`
    (_abi.make_plant_effects), `tau_ext` [B,n], `wrench` [B,6]: the saturated u plus the loads and the friction
    (include/abrk.h, abrk_plant_effects).  With all three None this is the plain entry point."""
    a = _Args(dtype, device)
    B = q.shape[0]
    qp, dqp, up = a.inp(q, (B, n), "q"), a.inp(dq, (B, n), "dq"), a.inp(u, (B, n), "u")
    if effects is None and tau_ext is None and wrench is None:
        op, oo = a.out(ddq, (B, n), "ddq")
        check(lib().abrk_forward_dynamics_batch(arm_id, a.code, B, qp, dqp, up, op, device, _sp(stream)))
        return oo
    ep, wp = a.inp(tau_ext, (B, n), "tau_ext"), a.inp(wrench, (B, 6), "wrench")
    op, oo = a.out(ddq, (B, n), "ddq")
    check(lib().abrk_forward_dynamics_fx_batch(arm_id, a.code, None if effects is None else C.byref(effects), B, qp,
                                               dqp, up, ep, wp, op, device, _sp(stream)))
    return oo


def plant_step(arm_id, n, params, q, dq, u, dtype=np.float64, device=0, stream=None, effects=None, tau_ext=None,
               wrench=None):
    """Rigid-body plant of any arm: (q, dq) [B,n] advanced in place by params.dt (_abi.make_plant_params) under the
    torques u [B,n].  `effects` (_abi.make_plant_effects: joint friction, limits, torque saturation), `tau_ext` [B,n] (a
    joint-space disturbance) and `wrench` [B,6] (a world-frame wrench at the end effector) make the plant non-ideal
    (include/abrk.h, abrk_plant_effects); with all three None this is the plain entry point.  Recorded into a plan, the
    contents of tau_ext and wrench are read at every replay."""
    a = _Args(dtype, device)
    B = q.shape[0]
    qp, dqp = a.inout(q, (B, n), "q"), a.inout(dq, (B, n), "dq")
    up = a.inp(u, (B, n), "u")
    if effects is None and tau_ext is None and wrench is None:
        check(lib().abrk_plant_step_batch(arm_id, a.code, C.byref(params), B, qp, dqp, up, device, _sp(stream)))
        return
    ep, wp = a.inp(tau_ext, (B, n), "tau_ext"), a.inp(wrench, (B, 6), "wrench")
    check(lib().abrk_plant_step_fx_batch(arm_id, a.code, C.byref(params), None if effects is None else C.byref(effects),
                                         B, qp, dqp, up, ep, wp, device, _sp(stream)))


def osc_rollout_twolink(arm_id, params, plant, q, dq, target, n_steps, every=0, integrated_error=None,
                        want_traj=False, dtype=np.float64, device=0, stream=None):
    """n_steps x { OSC.generate ; ArmSim._step } in one launch.  q, dq [B,2] are advanced in place.
    Returns (q_traj, dq_traj, u_traj) [B, n_steps // every, 2] when want_traj, else None."""
    a = _Args(dtype, device)
    B = q.shape[0]
    qp, dqp = a.inout(q, (B, 2), "q"), a.inout(dq, (B, 2), "dq")
    tp = a.inp(target, (B, 6), "target")
    iep = a.inout(integrated_error, (B, 6), "integrated_error")
    outs, ptrs = (None, None, None), (None, None, None)
    if want_traj:
        n_chk = n_steps // every if every else 0
        pairs = [a.out(None, (B, n_chk, 2), nm) for nm in ("q_traj", "dq_traj", "u_traj")]
        ptrs, outs = tuple(p for p, _ in pairs), tuple(o for _, o in pairs)
    check(lib().abrk_osc_rollout_twolink_batch(arm_id, a.code, C.byref(params), C.byref(plant), B, int(n_steps),
                                               int(every), qp, dqp, tp, iep, ptrs[0], ptrs[1], ptrs[2], device,
                                               _sp(stream)))
    return outs if want_traj else None


def _path_table(a, params, table, offsets):
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if offsets.shape != (2 + 4 * int(params.n_candidates),):
        raise ValueError(f"offsets: expected {2 + 4 * int(params.n_candidates)} entries, got {offsets.shape}")
    a.keep.append(offsets)
    if isinstance(table, DeviceArray):  # (the table may live on the device while the rows come from the host)
        if table.dtype != np.float64 or table.shape != (int(params.table_len),):
            raise ValueError("table: expected a float64 DeviceArray of table_len values")
        return table.ptr, offsets.ctypes.data
    t = np.ascontiguousarray(table, dtype=np.float64)
    if t.shape != (int(params.table_len),):
        raise ValueError(f"table: expected {int(params.table_len)} values, got {t.shape}")
    a.keep.append(t)
    return t.ctypes.data, offsets.ctypes.data


def path_plan(params, table, offsets, start, target, device=0, stream=None):
    """The plan pass of the batched PathPlanner (abrk_path_plan_batch): start, target [B,3] ->
    (n_timesteps [B] int32, rowplan [B,2] int32, dist_steps [B, n_samples]).  params: _abi.PathParams; table / offsets:
    the packed profile tables (controllers/path_planners/path_planner.py builds them).  Raises PathError (a ValueError)
    when a row has no path."""
    a = _Args(np.float64, device)
    B = start.shape[0]
    sp, tp = a.inp(start, (B, 3), "start"), a.inp(target, (B, 3), "target")
    tabp, offp = _path_table(a, params, table, offsets)
    if a.on_device:
        nt, rp = DeviceArray((B,), np.int32, device), DeviceArray((B, 2), np.int32, device)
        ntp, rpp = nt.ptr, rp.ptr
    else:
        nt, rp = np.zeros((B,), np.int32), np.zeros((B, 2), np.int32)
        ntp, rpp = nt.ctypes.data, rp.ctypes.data
    dsp, ds = a.out(None, (B, int(params.n_samples)), "dist_steps")
    check(lib().abrk_path_plan_batch(C.byref(params), tabp, offp, B, sp, tp, ntp, rpp, dsp, device, _sp(stream)))
    return nt, rp, ds


def path_fill(params, table, offsets, t_max, start, target, n_timesteps, rowplan, dist_steps, start_orientation=None,
              target_orientation=None, path=None, device=0, stream=None):
    """The fill and gradient passes (abrk_path_fill_batch) -> path [B, t_max, params.width]: row b is its path in
    [:n_timesteps[b]] and its last point after that.  A row with n_timesteps[b] == 0 or n_timesteps[b] > t_max is left
    as it was in every column: a path is never truncated."""
    a = _Args(np.float64, device)
    B = start.shape[0]
    sp, tp = a.inp(start, (B, 3), "start"), a.inp(target, (B, 3), "target")
    sop, top = a.inp(start_orientation, (B, 3), "start_orientation"), a.inp(target_orientation, (B, 3), "target_orientation")
    dsp = a.inp(dist_steps, (B, int(params.n_samples)), "dist_steps")
    ntp, rpp = a.side(n_timesteps, (B,), "n_timesteps"), a.side(rowplan, (B, 2), "rowplan")
    tabp, offp = _path_table(a, params, table, offsets)
    pp, po = a.out(path, (B, int(t_max), int(params.width)), "path")
    check(lib().abrk_path_fill_batch(C.byref(params), tabp, offp, B, int(t_max), sp, tp, sop, top, ntp, rpp, dsp, pp,
                                     device, _sp(stream)))
    return po


def path_next(path, n_timesteps, counter, target, target_velocity=None, dtype=np.float64, device=0, stream=None):
    """PathPlanner.next() for B rows as a kernel (abrk_path_next_batch) - recordable into a Plan: target[b] =
    path[b, counter[b], (0:3, 6:9)], target_velocity[b] = path[b, counter[b], (3:6, 9:12)], counter[b] advanced and
    clamped to n_timesteps[b] - 1.  path: float64 [B, Tmax, 6 | 12]; target / target_velocity: [B,6] of `dtype`, updated in
    place (a 6-wide path leaves their orientation columns alone); counter, n_timesteps: int32 [B]."""
    a = _Args(dtype, device)
    B, t_max, width = path.shape
    dev = isinstance(path, DeviceArray)
    a._mode(dev, "path")
    if path.dtype != np.float64 or (not dev and not path.flags.c_contiguous):
        raise ValueError("path: expected a C-contiguous float64 array [B, Tmax, W]")
    pp = path.ptr if dev else path.ctypes.data
    ntp, cp = a.side(n_timesteps, (B,), "n_timesteps"), a.side(counter, (B,), "counter")
    tgp = a.inout(target, (B, 6), "target")
    tvp = a.inout(target_velocity, (B, 6), "target_velocity")
    check(lib().abrk_path_next_batch(a.code, B, int(t_max), int(width), pp, ntp, cp, tgp, tvp, device, _sp(stream)))


def loop_trace(arm_id, n, params, q, dq, u, target, counter, history=None, stats=None, settle=None, dtype=np.float64,
               device=0, stream=None):
    """One tick of the loop recorder (abrk_loop_trace_batch) - recordable into a Plan.  With t = counter[b]: xyz =
    Tx(params.frame, params.x_off) of q[b], err = |target[b, :3] - xyz|; if t is a multiple of params.every and its slot
    t / every < params.capacity, the selected columns go to history[slot, b, :]; stats[b] = (err_last, err_max, err_min,
    err_sumsq) and settle[b] are updated; counter[b] = t + 1.  params: _abi.make_trace_params.  q, dq, u [B,n], target [B,6]
    of `dtype` (None where no selected output needs one); counter, settle: int32 [B]; history: [capacity, B, W] of `dtype`;
    stats: float64 [B,4].  counter, history, stats and settle are updated in place."""
    a = _Args(dtype, device)
    src = next((x for x in (q, target, dq, u) if x is not None), None)
    if src is None:
        raise ValueError("loop_trace needs at least one of q, dq, u, target")
    B = src.shape[0]
    qp, dqp, up = a.inp(q, (B, n), "q"), a.inp(dq, (B, n), "dq"), a.inp(u, (B, n), "u")
    tp = a.inp(target, (B, 6), "target")
    cp = a.side(counter, (B,), "counter")
    hp = sp = sep = None
    if history is not None:
        W = _abi.trace_layout(int(params.columns), n)[1]
        hp = a.inout(history, (int(params.capacity), B, W), "history")
    if stats is not None:
        sp = a.side(stats, (B, 4), "stats", np.float64)
    if settle is not None:
        sep = a.side(settle, (B,), "settle")
    check(lib().abrk_loop_trace_batch(arm_id, a.code, C.byref(params), B, qp, dqp, up, tp, cp, hp, sp, sep, device,
                                      _sp(stream)))


ADAPT_STATE = ("x_f", "e_f", "v", "ref", "a_f", "W", "out_f")


def adapt_state_shapes(params, B):
    """{name: shape} of the per-row state of engine.adapt_step for B rows"""
    D, O, N = int(params.n_input), int(params.n_output), int(params.n_neurons_total)
    return {"x_f": (B, D), "e_f": (B, O), "v": (B, N), "ref": (B, N), "a_f": (B, N), "W": (B, O, N), "out_f": (B, O)}


def adapt_step(params, enc, gain, bias, shift, scale, in0, training, state, in1=None, out=None, u_add=None,
               dtype=np.float64, device=0, stream=None):
    """One tick of the adaptive signal (abrk_adapt_step_batch) - recordable into a Plan.  params: _abi.make_adapt_params.
    enc [N,D], gain [N], bias [N], shift [D], scale [D] are shared by the rows; the row's input is concat(in0[b], in1[b])
    ([B,w0], [B,w1] with w0 + w1 = D: q and dq of a loop); training [B,O].  state: a dict of the seven arrays of
    adapt_state_shapes (v and ref may be missing for "lif_rate"), updated in place.  -> out [B,O], the filtered output;
    u_add [B,O], when given, has it added.  All arrays are of `dtype`, NumPy or DeviceArray alike."""
    a = _Args(dtype, device)
    D, O, N = int(params.n_input), int(params.n_output), int(params.n_neurons_total)
    B = in0.shape[0]
    w0 = in0.shape[1]
    w1 = 0 if in1 is None else in1.shape[1]
    i0p, i1p = a.inp(in0, (B, w0), "in0"), a.inp(in1, (B, w1), "in1")
    tp = a.inp(training, (B, O), "training")
    tabs = [a.inp(x, sh, nm) for x, sh, nm in ((enc, (N, D), "enc"), (gain, (N,), "gain"), (bias, (N,), "bias"),
                                               (shift, (D,), "shift"), (scale, (D,), "scale"))]
    st = _abi.AdaptState()
    for name, shape in adapt_state_shapes(params, B).items():
        arr = state.get(name)
        if arr is not None:
            setattr(st, name, a.inout(arr, shape, name))
    up = a.inout(u_add, (B, O), "u_add")
    op, oo = a.out(out, (B, O), "out")
    check(lib().abrk_adapt_step_batch(a.code, C.byref(params), B, *tabs, i0p, w0, i1p, w1, tp, C.byref(st), op, up,
                                      device, _sp(stream)))
    return oo


class Plan:
    """One control tick recorded as a launch plan (abrk_plan_begin .. abrk_plan_end): every engine call made inside
    the `with` block - on DeviceArrays, with this plan's device and stream - is validated and converted once and its
    kernel launch kept; `launch()` then only enqueues the recorded kernels, `launch_graph(repeat)` replays `repeat`
    ticks as one hipGraph launch.

        with engine.Plan(device, stream) as tick:
            engine.avoid_joint_limits_generate(n, lim, q, u=une, dtype=dt, device=device, stream=stream)
            engine.avoid_obstacles_generate(arm, n, obs, q, u=une, accumulate=True, ..., stream=stream)
            engine.osc_generate(arm, n, params, q, dq, target, u_null_ext=une, u=u, ..., stream=stream)
        tick.launch()

    The arrays must stay alive as long as the plan (results the engine allocates are returned to the caller as
    usual; `keep()` parks references on the plan)."""

    def __init__(self, device=0, stream=None):
        self.device, self.stream, self.id = device, stream, None
        self._keep = [stream]
        self._launch = lib().abrk_plan_launch

    def __enter__(self):
        check(lib().abrk_plan_begin(self.device, _sp(self.stream)))
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is not None:
            lib().abrk_plan_abort()
            return False
        self.id = check(lib().abrk_plan_end())
        return False

    def keep(self, *objs):
        self._keep.extend(objs)
        return self

    def launch(self):
        rc = self._launch(self.id)
        if rc < 0:
            check(rc)

    def launch_graph(self, repeat):
        """`repeat` consecutive launches as one hipGraph launch (needs a plan on an explicit stream)"""
        check(lib().abrk_plan_launch_graph(self.id, int(repeat)))

    def launch_repeat(self, repeat):
        """`repeat` consecutive plain launches enqueued by one C call (abrk_plan_launch_repeat)"""
        check(lib().abrk_plan_launch_repeat(self.id, int(repeat)))

    def close(self):
        pid, self.id = self.id, None
        if pid is not None:
            lib().abrk_plan_destroy(pid)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class OscPlan(Plan):
    """A validated, pre-converted OSC launch on fixed device buffers (abrk_osc_plan_create): `launch()`
    only enqueues the kernel on the plan's stream - the per-tick cost of a control loop whose state lives
    on the GPU.  All arrays must be DeviceArrays; update their contents between launches."""

    def __init__(self, arm_id, n, params, q, dq, target, u, target_velocity=None, integrated_error=None,
                 u_null_ext=None, training_signal=None, dtype=np.float64, device=0, stream=None):
        Plan.__init__(self, device, stream)
        m = _PlanArgs(dtype, device, stream)
        B, ptrs, _ = _bind_osc(m, n, q, dq, target, target_velocity, integrated_error, u_null_ext, u, training_signal)
        self._keep += [q, dq, target, target_velocity, integrated_error, u_null_ext, u, training_signal, params]
        self.id = check(lib().abrk_osc_plan_create(arm_id, m.code, C.byref(params), B, *ptrs, *m.where))


class SlidingPlan(Plan):
    """The same for Sliding.generate (abrk_sliding_plan_create): launch(), launch_graph(repeat)"""

    def __init__(self, arm_id, n, params, q, dq, target, u, target_velocity=None, target_acc=None, s=None,
                 dtype=np.float64, device=0, stream=None):
        Plan.__init__(self, device, stream)
        m = _PlanArgs(dtype, device, stream)
        B, ptrs, _ = _bind_sliding(m, n, params, q, dq, target, target_velocity, target_acc, u, s)
        self._keep += [q, dq, target, target_velocity, target_acc, u, s, params]
        self.id = check(lib().abrk_sliding_plan_create(arm_id, m.code, C.byref(params), B, *ptrs, *m.where))


class MergedLoops:
    """Several INDEPENDENT control loops that run the same controller on one GPU, evaluated by ONE launch per tick.

    Why: independent loops on streams of their own do not overlap beyond two streams - the runtime maps streams onto a
    few hardware queues and the command processor serialises the dependent kernel chains that share one (measured,
    profiles/round6/concurrent_streams.md: 16 streams of 4096-row graph replays reach 3.0 G evaluations/s, while the
    same 65 536 rows as one launch take 5.4 us: 12.2 G/s; more hardware queues - GPU_MAX_HW_QUEUES=8 / 16 - make it
    4x WORSE).  A config-sized step occupies 64 of the chip's 1024 SIMDs, so the remedy is to put the loops' rows into
    one batch: loop i owns rows [lo_i, hi_i) of shared q / dq / target / u buffers (`loop(i)`: DeviceArray VIEWS - each
    loop writes its states and reads its torques without knowing of the others), and `launch()` / `launch_graph(K)`
    evaluate every loop's rows together.  The loops share the controller's parameters (one `abrk_osc_params` per
    launch); loops with different gains need launches of their own.

        loops = engine.MergedLoops(rc.arm_id, rc.N_JOINTS, params, [4096] * 16, device=0)
        loops.loop(3).q.copy_from_numpy(q3) ...        # every loop feeds its own rows
        loops.launch(); loops.stream.sync()
        u3 = loops.loop(3).u.numpy(loops.stream)"""

    def __init__(self, arm_id, n, params, rows_per_loop, dtype=np.float64, device=0, stream=None, target_velocity=False,
                 training_signal=False):
        from ._lib import Stream

        self.rows = [int(r) for r in rows_per_loop]
        if not self.rows or min(self.rows) < 1:
            raise ValueError("every loop needs at least one row")
        self.bounds = np.concatenate([[0], np.cumsum(self.rows)]).tolist()
        B = self.bounds[-1]
        self.device, self.stream = device, stream if stream is not None else Stream(device)
        mk = lambda w: DeviceArray((B, w), dtype, device)
        self.q, self.dq, self.target, self.u = mk(n), mk(n), mk(6), mk(n)
        self.target_velocity = mk(6).zero_() if target_velocity else None
        self.integrated_error = mk(6).zero_() if params.ki != 0 else None
        self.training_signal = mk(n) if training_signal else None
        with Plan(device, self.stream) as self.plan:
            osc_generate(arm_id, n, params, self.q, self.dq, self.target, self.target_velocity, self.integrated_error,
                         None, self.u, self.training_signal if training_signal else False, dtype=dtype, device=device,
                         stream=self.stream)

    def loop(self, i):
        """loop i's rows of every buffer, as DeviceArray views: .q .dq .target .u (.target_velocity .integrated_error
        .training_signal where present)"""
        import types

        lo, hi = self.bounds[i], self.bounds[i + 1]
        v = lambda a: None if a is None else a.rows(lo, hi)
        return types.SimpleNamespace(q=v(self.q), dq=v(self.dq), target=v(self.target), u=v(self.u),
                                     target_velocity=v(self.target_velocity), integrated_error=v(self.integrated_error),
                                     training_signal=v(self.training_signal), rows=(lo, hi))

    def launch(self):
        self.plan.launch()

    def launch_graph(self, repeat):
        self.plan.launch_graph(repeat)

    def close(self):
        self.plan.close()


def ik_generate_path(arm_id, n, params, position, target, dtype=np.float64, device=0, stream=None,
                     position_path=None, velocity_path=None):
    """InverseKinematics.generate_path for B paths: position [B,n], target [B,6] (xyz + Euler 'sxyz').
    Returns (position_path, velocity_path), each [B, n_timesteps, n]."""
    a = _Args(dtype, device)
    B = position.shape[0]
    T = int(params.n_timesteps)
    qp = a.inp(position, (B, n), "position")
    tp = a.inp(target, (B, 6), "target")
    ppp, ppo = a.out(position_path, (B, T, n), "position_path")
    vpp, vpo = a.out(velocity_path, (B, T, n), "velocity_path")
    check(lib().abrk_ik_generate_path_batch(arm_id, a.code, C.byref(params), B, qp, tp, ppp, vpp, device, _sp(stream)))
    return ppo, vpo
