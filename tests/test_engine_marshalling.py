"""What the Python call layer hands to libabrk.so, pinned without a device and without the library: a recording
fake stands in for `lib()`, and every public entry of engine.py - on NumPy arrays, on DeviceArrays, sharded over
devices, on resident shards, as a plan - is checked for the C function it calls, each scalar by value, each pointer by
the array it belongs to, the fields of the structs it passes by reference, what it returns and what it refuses.  The
expected values are written out here; nothing is computed by the code under test."""
import ctypes as C
import inspect
import weakref

import numpy as np
import pytest

from abr_control_amd import _abi, _lib, engine, sharding
from abr_control_amd._lib import DeviceArray
from abr_control_amd.sharding import MultiDevice, ShardedArray

B, N, ARM = 3, 6, 7
DTYPES = [np.float64, np.float32]
CODE = {np.float64: _abi.F64, np.float32: _abi.F32}
DYN_FIELDS = ("Tx", "J", "M", "g", "C", "dJ", "R", "T", "Tinv", "quat")
DYN_SHAPES = {"Tx": (3,), "J": (6, N), "M": (N, N), "g": (N,), "C": (N, N), "dJ": (6, N), "R": (3, 3), "T": (4, 4),
              "Tinv": (4, 4), "quat": (4,)}
DYN_BITS = {"Tx": 1, "J": 2, "M": 4, "g": 8, "C": 16, "dJ": 32, "R": 64, "T": 128, "Tinv": 256, "quat": 512}


class FakeLib:
    """every attribute is a function that records (name, args) and returns 0 - but for the three that must answer"""

    def __init__(self):
        self.calls, self.issued, self.hook, self._next = [], set(), None, 0x10000

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if self.hook is not None:
                self.hook(name, args)
            if name == "abrk_malloc":
                self._next += 0x10000
                self.issued.add(self._next)
                return self._next
            if name == "abrk_shard_stream":
                return 0x5000 + 0x100 * args[0] + args[1]
            if name == "abrk_device_count":
                return 8
            return 0

        fn.fake = self
        return fn

    def last(self, prefix="abrk_"):
        skip = ("abrk_malloc", "abrk_free", "abrk_memset", "abrk_memcpy_h2d", "abrk_memcpy_d2h", "abrk_shard_stream",
                "abrk_device_count")
        return next(c for c in reversed(self.calls) if c[0].startswith(prefix) and c[0] not in skip)

    def named(self, name):
        return [c for c in self.calls if c[0] == name]


@pytest.fixture
def fake(monkeypatch):
    f = FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: f)
    monkeypatch.setattr(engine, "lib", lambda: f)
    made = []
    for cls in (DeviceArray, engine.Plan):
        def init(self, *a, _init=cls.__init__, **kw):
            made.append(weakref.ref(self))
            _init(self, *a, **kw)
        monkeypatch.setattr(cls, "__init__", init)
    yield f
    # nothing made under the fake may reach the real library when it is collected later
    for o in filter(None, (r() for r in made)):
        if isinstance(o, DeviceArray):
            o.ptr = None
        else:
            o.id = None


class Stream:
    ptr = 0x77


def host(shape, dtype, fill=0.5):
    return np.full(shape, fill, dtype)


def dev(shape, dtype, device=0):
    return DeviceArray(shape, dtype, device)


FORMS = {"numpy": host, "device": lambda shape, dtype, fill=0.0: dev(shape, dtype, 2)}
KIND = {"numpy": np.ndarray, "device": DeviceArray}


def addr(x):
    if x is None:
        return None
    return x.ptr if isinstance(x, DeviceArray) else x.ctypes.data


def tab(x):
    return None if x is None else tuple(p.ptr for p in x.parts)


def ref(s):
    return ("ref", C.addressof(s))


def norm(args):
    """byref(struct) -> ("ref", address); a ctypes array of numbers or pointers -> a tuple; the rest as it is"""
    out = []
    for a in args:
        if hasattr(a, "_obj"):
            out.append(("ref", C.addressof(a._obj)))
        elif isinstance(a, C.Array) and issubclass(a._type_, C._SimpleCData):
            out.append(tuple(a))
        else:
            out.append(a)
    return tuple(out)


def is_arr(x, kind, shape, dtype):
    return type(x) is kind and tuple(x.shape) == tuple(shape) and x.dtype == np.dtype(dtype)


def dyn_out(do, res):
    return {k: getattr(do, k) for k in DYN_FIELDS} == {k: addr(res.get(k)) for k in DYN_FIELDS}


def cut_of(arg):
    c = arg._obj
    G = c.n_shards
    return G, [c.devices[g] for g in range(G)], [c.rows[g] for g in range(G)], \
        None if not c.streams else [c.streams[g] for g in range(G)]


# ---------------------------------------------------------------------------- dynamics
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["numpy", "device"])
def test_dynamics(fake, form, dtype):
    A = FORMS[form]
    q, dq = A((B, N), dtype), A((B, N), dtype)
    want = ("Tx", "J", "M", "g")
    given = A((B, N, N), dtype)
    res = engine.dynamics(ARM, N, q, dq, 5, [0.1, 0.2, 0.3], want, dtype, 2, Stream(), out={"M": given})
    name, args = fake.last()
    assert name == "abrk_dynamics_batch" and len(args) == 11
    assert args[:6] == (ARM, CODE[dtype], B, addr(q), addr(dq), 5) and list(args[6]) == [0.1, 0.2, 0.3]
    assert args[7] == 1 | 2 | 4 | 8 and dyn_out(args[8]._obj, res) and args[9:] == (2, 0x77)
    assert list(res) == list(want) and res["M"] is given
    assert all(is_arr(res[k], KIND[form], (B,) + DYN_SHAPES[k], dtype) for k in want)
    # the defaults: the end effector's frame, no offset, no velocities, M alone, device 0, the NULL stream
    res = engine.dynamics(ARM, N, q, dtype=dtype)
    name, args = fake.last()
    assert args[:8] == (ARM, CODE[dtype], B, addr(q), None, 2 * N + 1, None, 4) and args[9:] == (0, None)
    assert list(res) == ["M"] and dyn_out(args[8]._obj, res)
    # every output has its bit and its shape
    res = engine.dynamics(ARM, N, q, dq, want=DYN_FIELDS, dtype=dtype)
    name, args = fake.last()
    assert args[7] == 1023 and dyn_out(args[8]._obj, res)
    assert all(tuple(res[k].shape) == (B,) + DYN_SHAPES[k] for k in DYN_FIELDS)
    assert all(1 << i == DYN_BITS[k] for i, k in enumerate(DYN_FIELDS))
    with pytest.raises(KeyError, match="nope"):
        engine.dynamics(ARM, N, q, want=("nope",), dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dynamics_sharded_and_resident(fake, dtype):
    q, dq = host((B, N), dtype), host((B, N), dtype)
    res = engine.dynamics_sharded(ARM, N, q, [0, 1, 1], dq, 4, [1, 2, 3], ("Tx", "C"), dtype)
    name, args = fake.last()
    assert name == "abrk_dynamics_sharded" and len(args) == 11
    assert norm(args)[:6] == (ARM, CODE[dtype], B, addr(q), addr(dq), 4) and list(args[6]) == [1.0, 2.0, 3.0]
    assert args[7] == 1 | 16 and dyn_out(args[8]._obj, res) and norm(args)[9:] == (3, (0, 1, 1))
    assert list(res) == ["Tx", "C"] and all(is_arr(res[k], np.ndarray, (B,) + DYN_SHAPES[k], dtype) for k in res)
    with pytest.raises(TypeError, match="q"):
        engine.dynamics_sharded(ARM, N, dev((B, N), dtype), [0], dtype=dtype)

    devices = [0, 1, 1]
    qs, dqs = ShardedArray.empty((5, N), dtype, devices), ShardedArray.empty((5, N), dtype, devices)
    given = ShardedArray.empty((5, N), dtype, devices)
    res = engine.dynamics_resident(ARM, N, qs, dqs, None, None, ("g", "M"), dtype, [0x11, Stream(), None], {"g": given})
    name, args = fake.last()
    assert name == "abrk_dynamics_resident" and len(args) == 9
    assert norm(args)[:2] == (ARM, CODE[dtype]) and cut_of(args[2]) == (3, devices, [2, 2, 1], [0x11, 0x77, None])
    assert norm(args)[3:8] == (tab(qs), tab(dqs), 2 * N + 1, None, 8 | 4)
    assert len(args[8]) == 3 and res["g"] is given and list(res) == ["g", "M"]
    for g in range(3):
        assert {k: getattr(args[8][g], k) for k in DYN_FIELDS} == {
            k: res[k].parts[g].ptr if k in res else None for k in DYN_FIELDS}
    assert type(res["M"]) is ShardedArray and res["M"].shape == (5, N, N) and res["M"].dtype == np.dtype(dtype)
    assert res["M"].devices == devices and res["M"].rows == [2, 2, 1]
    with pytest.raises(ValueError, match="dq"):
        engine.dynamics_resident(ARM, N, qs, ShardedArray.empty((5, N), dtype, [0, 1, 2]), dtype=dtype)


# ---------------------------------------------------------------------------- OSC
def osc_args(q, dq, t, tv, ie, une, u, ts):
    return tuple(addr(x) for x in (q, dq, t, tv, ie, une, u, ts))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["numpy", "device"])
def test_osc_generate(fake, form, dtype):
    A = FORMS[form]
    p = _abi.make_osc_params(N, kp=50, ki=0.1)
    q, dq, t, tv, ie, une = (A(s, dtype) for s in ((B, N), (B, N), (B, 6), (B, 6), (B, 6), (B, N)))
    u = engine.osc_generate(ARM, N, p, q, dq, t, dtype=dtype)
    name, args = fake.last()
    assert name == "abrk_osc_generate_batch" and len(args) == 14
    assert norm(args) == (ARM, CODE[dtype], ref(p), B) + osc_args(q, dq, t, None, None, None, u, None) + (0, None)
    assert is_arr(u, KIND[form], (B, N), dtype)
    ug, tsg = A((B, N), dtype), A((B, N), dtype)
    r = engine.osc_generate(ARM, N, p, q, dq, t, tv, ie, une, ug, tsg, dtype, 2, Stream())
    name, args = fake.last()
    assert norm(args) == (ARM, CODE[dtype], ref(p), B) + osc_args(q, dq, t, tv, ie, une, ug, tsg) + (2, 0x77)
    assert type(r) is tuple and r[0] is ug and r[1] is tsg
    u, ts = engine.osc_generate(ARM, N, p, q, dq, t, training_signal=True, dtype=dtype, device=2)
    name, args = fake.last()
    assert norm(args)[4:] == osc_args(q, dq, t, None, None, None, u, ts) + (2, None)
    assert is_arr(ts, KIND[form], (B, N), dtype) and addr(ts) != addr(u)
    assert type(engine.osc_generate(ARM, N, p, q, dq, t, training_signal=None, dtype=dtype, device=2)) is KIND[form]
    # the fused robot_config outputs
    given = A((B, 6, N), dtype)
    u, res = engine.osc_generate(ARM, N, p, q, dq, t, tv, ie, dtype=dtype, device=2, want=("Tx", "J"), out={"J": given})
    name, args = fake.last()
    assert name == "abrk_osc_generate_full_batch" and len(args) == 16
    assert norm(args)[:12] == (ARM, CODE[dtype], ref(p), B) + osc_args(q, dq, t, tv, ie, None, u, None)
    assert args[12] == 3 and dyn_out(args[13]._obj, res) and args[14:] == (2, None)
    assert list(res) == ["Tx", "J"] and res["J"] is given and is_arr(res["Tx"], KIND[form], (B, 3), dtype)
    r = engine.osc_generate(ARM, N, p, q, dq, t, training_signal=True, dtype=dtype, device=2, want=("M",))
    assert len(r) == 3 and type(r[2]) is dict and fake.last()[1][11] == addr(r[1])
    with pytest.raises(ValueError, match="quat"):
        engine.osc_generate(ARM, N, p, q, dq, t, dtype=dtype, device=2, want=("quat",))


@pytest.mark.parametrize("dtype", DTYPES)
def test_osc_generate_refusals(fake, dtype):
    p = _abi.make_osc_params(N, kp=50, ki=0.1)
    other = np.float32 if dtype is np.float64 else np.float64
    q, dq, t = host((B, N), dtype), host((B, N), dtype), host((B, 6), dtype)
    qd, dqd, td = dev((B, N), dtype), dev((B, N), dtype), dev((B, 6), dtype)
    n0 = len(fake.calls)
    with pytest.raises(ValueError, match="dq"):
        engine.osc_generate(ARM, N, p, q, host((B, N + 1), dtype), t, dtype=dtype)
    with pytest.raises(ValueError, match="target"):
        engine.osc_generate(ARM, N, p, qd, dqd, dev((B, 3), dtype), dtype=dtype)
    with pytest.raises(ValueError, match="target_velocity"):
        engine.osc_generate(ARM, N, p, qd, dqd, td, dev((B, 6), other), dtype=dtype)
    with pytest.raises(TypeError, match="mixing"):
        engine.osc_generate(ARM, N, p, q, dqd, t, dtype=dtype)
    with pytest.raises(TypeError, match="mixing"):
        engine.osc_generate(ARM, N, p, qd, dqd, td, integrated_error=host((B, 6), dtype), dtype=dtype)
    for bad in (host((B, 6), other), host((B, 5), dtype), host((6, B), dtype).T, [[0.0] * 6] * B):
        with pytest.raises(ValueError, match="integrated_error"):
            engine.osc_generate(ARM, N, p, q, dq, t, integrated_error=bad, dtype=dtype)
    for bad in (host((B, N), other), host((N, B), dtype).T, host((B, N + 1), dtype), dev((B, N), dtype)):
        with pytest.raises(ValueError, match="u"):
            engine.osc_generate(ARM, N, p, q, dq, t, u=bad, dtype=dtype)
    with pytest.raises(ValueError, match="training_signal"):
        engine.osc_generate(ARM, N, p, qd, dqd, td, training_signal=host((B, N), dtype), dtype=dtype)
    with pytest.raises(TypeError, match="float"):
        engine.osc_generate(ARM, N, p, q, dq, t, dtype=np.float16)
    assert not [c for c in fake.calls[n0:] if c[0].startswith("abrk_osc")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["numpy", "device"])
def test_osc_generate_coop_and_helpers(fake, form, dtype):
    A = FORMS[form]
    p = _abi.make_osc_params(N, kp=50, vmax=[0.5, 1.0])
    q, dq, t = A((B, N), dtype), A((B, N), dtype), A((B, 6), dtype)
    u, ts = engine.osc_generate_coop(ARM, N, p, q, dq, t, 8, None, True, dtype, 2, Stream())
    name, args = fake.last()
    assert name == "abrk_osc_generate_coop_batch"
    assert norm(args) == (ARM, CODE[dtype], ref(p), B, addr(q), addr(dq), addr(t), addr(u), addr(ts), 8, 2, 0x77)
    ug = A((B, N), dtype)
    assert engine.osc_generate_coop(ARM, N, p, q, dq, t, 4, ug, dtype=dtype, device=2) is ug
    assert norm(fake.last()[1])[7:] == (addr(ug), None, 4, 2, None)

    M, J = A((B, N, N), dtype), A((B, 3, N), dtype)
    Mx, Minv = engine.osc_mx(N, M, J, 0.01, True, dtype, 2, Stream())
    name, args = fake.last()
    assert name == "abrk_osc_mx_batch"
    assert args == (N, 3, CODE[dtype], B, addr(M), addr(J), 0.01, addr(Mx), addr(Minv), 2, 0x77)
    assert is_arr(Mx, KIND[form], (B, 3, 3), dtype) and is_arr(Minv, KIND[form], (B, N, N), dtype)
    Mx, Minv = engine.osc_mx(N, M, J, want_minv=False, dtype=dtype, device=2)
    assert Minv is None and fake.last()[1][6:] == (1e-3, addr(Mx), None, 2, None)
    with pytest.raises(ValueError, match="J"):
        engine.osc_mx(N, M, A((B, 3, N + 1), dtype), dtype=dtype, device=2)

    ut = A((B, 6), dtype)
    o = engine.osc_velocity_limiting(p, ut, dtype, 2, Stream())
    name, args = fake.last()
    assert name == "abrk_osc_velocity_limiting_batch"
    assert norm(args) == (CODE[dtype], ref(p), B, addr(ut), addr(o), 2, 0x77) and is_arr(o, KIND[form], (B, 6), dtype)
    with pytest.raises(ValueError, match="u_task"):
        engine.osc_velocity_limiting(p, A((B, 5), dtype), dtype, 2)

    R, abg = A((B, 3, 3), dtype), A((B, 3), dtype)
    o = engine.osc_orientation_forces(1, R, abg, dtype, 2, Stream())
    name, args = fake.last()
    assert name == "abrk_osc_orientation_forces_batch"
    assert args == (1, CODE[dtype], B, addr(R), addr(abg), addr(o), 2, 0x77) and is_arr(o, KIND[form], (B, 3), dtype)
    with pytest.raises(ValueError, match="target_abg"):
        engine.osc_orientation_forces(1, R, A((B, 4), dtype), dtype, 2)

    a, b = A((B, 4), dtype), A((B, 4), dtype)
    o = engine.transformations(3, a, b, dtype, 2, Stream())
    name, args = fake.last()
    assert name == "abrk_transformations_batch"
    assert args == (3, CODE[dtype], B, addr(a), addr(b), addr(o), 2, 0x77) and is_arr(o, KIND[form], (B, 4), dtype)
    o = engine.transformations(7, A((B, 3), dtype), dtype=dtype, device=2)
    assert fake.last()[1][4] is None and tuple(o.shape) == (B, 9)
    with pytest.raises(ValueError, match="a"):
        engine.transformations(2, a, dtype=dtype, device=2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["numpy", "device"])
def test_osc_law(fake, form, dtype):
    A = FORMS[form]
    p = _abi.make_osc_params(N, kp=50, ki=0.1)
    J, M, g, Cdq, xyz, R = (A(s, dtype) for s in ((B, 6, N), (B, N, N), (B, N), (B, N), (B, 3), (B, 3, 3)))
    q, dq, t, tv, ie, une = (A(s, dtype) for s in ((B, N), (B, N), (B, 6), (B, 6), (B, 6), (B, N)))
    u, ts = engine.osc_law(N, p, J, M, dq, t, g, Cdq, xyz, R, q, tv, ie, une, True, dtype, 2, Stream())
    name, args = fake.last()
    assert name == "abrk_osc_law_batch" and len(args) == 20
    assert norm(args) == (N, CODE[dtype], ref(p), B) + tuple(addr(x) for x in (
        J, M, g, Cdq, xyz, R, q, dq, t, tv, ie, une, u, ts)) + (2, 0x77)
    assert is_arr(u, KIND[form], (B, N), dtype) and is_arr(ts, KIND[form], (B, N), dtype)
    u = engine.osc_law(N, p, J, M, dq, t, dtype=dtype, device=2)
    assert norm(fake.last()[1])[4:] == (addr(J), addr(M)) + (None,) * 5 + (addr(dq), addr(t), None, None, None,
                                                                          addr(u), None, 2, None)
    assert type(u) is KIND[form]
    if form == "device":  # training_signal is a flag here: any true value asks for a fresh array
        r = engine.osc_law(N, p, J, M, dq, t, training_signal=une, dtype=dtype, device=2)
        assert r[1] is not une and is_arr(r[1], DeviceArray, (B, N), dtype) and fake.last()[1][17] == addr(r[1])
    with pytest.raises(ValueError, match="Cdq"):
        engine.osc_law(N, p, J, M, dq, t, Cdq=A((B, N + 1), dtype), dtype=dtype, device=2)
    with pytest.raises(ValueError, match="integrated_error"):
        engine.osc_law(N, p, J, M, dq, t, integrated_error=A((B, 5), dtype), dtype=dtype, device=2)
    if form == "numpy":
        with pytest.raises(ValueError, match="integrated_error"):
            engine.osc_law(N, p, J, M, dq, t, integrated_error=host((6, B), dtype).T, dtype=dtype)
        with pytest.raises(TypeError, match="mixing"):
            engine.osc_law(N, p, J, M, dq, t, integrated_error=dev((B, 6), dtype), dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_osc_law_refuses_a_numpy_state_beside_device_inputs(fake, dtype):
    """as osc_generate does (the copy of the check that osc_law had of its own forgot the mode)"""
    p = _abi.make_osc_params(N, kp=50, ki=0.1)
    J, M, dq, t = (dev(s, dtype) for s in ((B, 6, N), (B, N, N), (B, N), (B, 6)))
    with pytest.raises(TypeError, match="mixing DeviceArray and NumPy"):
        engine.osc_law(N, p, J, M, dq, t, integrated_error=host((B, 6), dtype), dtype=dtype)
    assert not fake.named("abrk_osc_law_batch")


@pytest.mark.parametrize("dtype", DTYPES)
def test_osc_generate_sharded_and_resident(fake, dtype):
    p = _abi.make_osc_params(N, kp=50, ki=0.1)
    q, dq, t, tv, ie, une = (host(s, dtype) for s in ((B, N), (B, N), (B, 6), (B, 6), (B, 6), (B, N)))
    u = engine.osc_generate_sharded(ARM, N, p, q, dq, t, [0, 0, 1], dtype=dtype)
    name, args = fake.last()
    assert name == "abrk_osc_generate_sharded" and len(args) == 14
    assert norm(args) == (ARM, CODE[dtype], ref(p), B) + osc_args(q, dq, t, None, None, None, u, None) + (3, (0, 0, 1))
    assert is_arr(u, np.ndarray, (B, N), dtype)
    ug = host((B, N), dtype)
    r = engine.osc_generate_sharded(ARM, N, p, q, dq, t, (np.int64(1), 0), tv, ie, une, ug, True, dtype)
    name, args = fake.last()
    assert norm(args) == (ARM, CODE[dtype], ref(p), B) + osc_args(q, dq, t, tv, ie, une, ug, r[1]) + (2, (1, 0))
    assert r[0] is ug and is_arr(r[1], np.ndarray, (B, N), dtype)
    for k, name_ in enumerate(("q", "dq", "target")):
        a = [q, dq, t]
        a[k] = dev(a[k].shape, dtype)
        with pytest.raises(TypeError, match=name_):
            engine.osc_generate_sharded(ARM, N, p, a[0], a[1], a[2], [0], dtype=dtype)
    for kw in ("target_velocity", "u_null_ext", "u"):
        with pytest.raises(TypeError, match=kw):
            engine.osc_generate_sharded(ARM, N, p, q, dq, t, [0], dtype=dtype, **{kw: dev((B, 6), dtype)})
    # (a DeviceArray state or training_signal was refused as a ValueError before the sharded calls had one marshaller)
    for kw in ("integrated_error", "training_signal"):
        with pytest.raises((TypeError, ValueError), match=kw):
            engine.osc_generate_sharded(ARM, N, p, q, dq, t, [0], dtype=dtype, **{kw: dev((B, 6), dtype)})
    assert len(fake.named("abrk_osc_generate_sharded")) == 2
    with pytest.raises(ValueError, match="integrated_error"):
        engine.osc_generate_sharded(ARM, N, p, q, dq, t, [0], integrated_error=host((6, B), dtype).T, dtype=dtype)
    with pytest.raises(ValueError, match="target"):
        engine.osc_generate_sharded(ARM, N, p, q, dq, host((B, 5), dtype), [0], dtype=dtype)

    devices = [0, 1, 1, 2]
    S = lambda *tail: ShardedArray.empty((9,) + tail, dtype, devices)
    qs, dqs, ts_, tvs, ies, unes, us = S(N), S(N), S(6), S(6), S(6), S(N), S(N)
    u = engine.osc_generate_resident(ARM, N, p, qs, dqs, ts_, dtype=dtype)
    name, args = fake.last()
    assert name == "abrk_osc_generate_resident" and len(args) == 12
    assert norm(args)[:3] == (ARM, CODE[dtype], ref(p)) and cut_of(args[3]) == (4, devices, [3, 2, 2, 2], None)
    assert norm(args)[4:] == (tab(qs), tab(dqs), tab(ts_), None, None, None, tab(u), None)
    assert type(u) is ShardedArray and u.shape == (9, N) and u.dtype == np.dtype(dtype) and u.devices == devices
    streams = [Stream(), 0x21, 0x22, 0x23]
    r = engine.osc_generate_resident(ARM, N, p, qs, dqs, ts_, tvs, ies, unes, us, True, dtype, streams)
    name, args = fake.last()
    assert cut_of(args[3]) == (4, devices, [3, 2, 2, 2], [0x77, 0x21, 0x22, 0x23])
    assert norm(args)[4:] == (tab(qs), tab(dqs), tab(ts_), tab(tvs), tab(ies), tab(unes), tab(us), tab(r[1]))
    assert r[0] is us and type(r[1]) is ShardedArray and r[1].rows == [3, 2, 2, 2]
    tsg = S(N)
    assert engine.osc_generate_resident(ARM, N, p, qs, dqs, ts_, training_signal=tsg, dtype=dtype)[1] is tsg
    other = ShardedArray.empty((9, N), dtype, [0, 1, 2, 2])
    with pytest.raises(ValueError, match="dq"):
        engine.osc_generate_resident(ARM, N, p, qs, other, ts_, dtype=dtype)
    with pytest.raises(ValueError, match="u_null_ext"):
        engine.osc_generate_resident(ARM, N, p, qs, dqs, ts_, u_null_ext=ShardedArray.empty((9, N), dtype, devices,
                                                                                             rows=[2, 3, 2, 2]), dtype=dtype)
    with pytest.raises(ValueError, match="target"):
        engine.osc_generate_resident(ARM, N, p, qs, dqs, S(3), dtype=dtype)
    with pytest.raises(ValueError, match="streams"):
        engine.osc_generate_resident(ARM, N, p, qs, dqs, ts_, dtype=dtype, streams=[1, 2])
    engine.shards_sync(qs, streams)
    name, args = fake.last()
    assert name == "abrk_shards_sync" and cut_of(args[0]) == (4, devices, [3, 2, 2, 2], [0x77, 0x21, 0x22, 0x23])


# ---------------------------------------------------------------------------- Sliding, Joint
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cartesian", [True, False])
def test_sliding_every_form(fake, cartesian, dtype):
    p = _abi.make_sliding_params(N, 100.0, 20.0, cartesian)
    nt = 3 if cartesian else N
    for form, A in FORMS.items():
        q, dq, t, tv, ta = (A(s, dtype) for s in ((B, N), (B, N), (B, nt), (B, nt), (B, nt)))
        u = engine.sliding_generate(ARM, N, p, q, dq, t, dtype=dtype, device=2)
        name, args = fake.last()
        assert name == "abrk_sliding_generate_batch" and len(args) == 13
        assert norm(args) == (ARM, CODE[dtype], ref(p), B, addr(q), addr(dq), addr(t), None, None, addr(u), None, 2, None)
        assert is_arr(u, KIND[form], (B, N), dtype)
        ug = A((B, N), dtype)
        r = engine.sliding_generate(ARM, N, p, q, dq, t, tv, ta, ug, True, dtype, 2, Stream())
        assert norm(fake.last()[1])[4:] == (addr(q), addr(dq), addr(t), addr(tv), addr(ta), addr(ug), addr(r[1]), 2, 0x77)
        assert r[0] is ug and is_arr(r[1], KIND[form], (B, N), dtype)
        with pytest.raises(ValueError, match="target_acc"):
            engine.sliding_generate(ARM, N, p, q, dq, t, tv, A((B, nt + 1), dtype), dtype=dtype, device=2)
        if form == "device":  # want_s is a flag here: any true value asks for a fresh array
            sg = A((B, N), dtype)
            r = engine.sliding_generate(ARM, N, p, q, dq, t, want_s=sg, dtype=dtype, device=2)
            assert r[1] is not sg and is_arr(r[1], DeviceArray, (B, N), dtype) and fake.last()[1][10] == addr(r[1])
    q, dq, t, tv, ta = (host(s, dtype) for s in ((B, N), (B, N), (B, nt), (B, nt), (B, nt)))
    u, s = engine.sliding_generate_sharded(ARM, N, p, q, dq, t, [1, 0], tv, ta, True, dtype)
    name, args = fake.last()
    assert name == "abrk_sliding_generate_sharded" and len(args) == 13
    assert norm(args) == (ARM, CODE[dtype], ref(p), B, addr(q), addr(dq), addr(t), addr(tv), addr(ta), addr(u), addr(s),
                          2, (1, 0))
    assert is_arr(u, np.ndarray, (B, N), dtype) and is_arr(s, np.ndarray, (B, N), dtype)
    u = engine.sliding_generate_sharded(ARM, N, p, q, dq, t, [1], dtype=dtype)
    assert norm(fake.last()[1])[7:] == (None, None, addr(u), None, 1, (1,)) and type(u) is np.ndarray
    for kw in ("target_velocity", "target_acc"):
        with pytest.raises(TypeError, match=kw):
            engine.sliding_generate_sharded(ARM, N, p, q, dq, t, [0], dtype=dtype, **{kw: dev((B, nt), dtype)})
    with pytest.raises(TypeError, match="dq"):
        engine.sliding_generate_sharded(ARM, N, p, q, dev((B, N), dtype), t, [0], dtype=dtype)

    devices = [0, 1]
    S = lambda *tail: ShardedArray.empty((5,) + tail, dtype, devices)
    qs, dqs, ts_, tvs, tas, us = S(N), S(N), S(nt), S(nt), S(nt), S(N)
    r = engine.sliding_generate_resident(ARM, N, p, qs, dqs, ts_, tvs, tas, us, True, dtype, [0x31, 0x32])
    name, args = fake.last()
    assert name == "abrk_sliding_generate_resident" and len(args) == 11
    assert norm(args)[:3] == (ARM, CODE[dtype], ref(p)) and cut_of(args[3]) == (2, devices, [3, 2], [0x31, 0x32])
    assert norm(args)[4:] == (tab(qs), tab(dqs), tab(ts_), tab(tvs), tab(tas), tab(us), tab(r[1]))
    assert r[0] is us and type(r[1]) is ShardedArray and r[1].shape == (5, N)
    sg = S(N)
    assert engine.sliding_generate_resident(ARM, N, p, qs, dqs, ts_, want_s=sg, dtype=dtype)[1] is sg
    u = engine.sliding_generate_resident(ARM, N, p, qs, dqs, ts_, dtype=dtype)
    assert norm(fake.last()[1])[7:] == (None, None, tab(u), None) and type(u) is ShardedArray
    with pytest.raises(ValueError, match="target_velocity"):
        engine.sliding_generate_resident(ARM, N, p, qs, dqs, ts_, ShardedArray.empty((5, nt), dtype, [1, 0]), dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_joint_every_form(fake, dtype):
    c = _abi.make_joint(20, 4)
    for form, A in FORMS.items():
        q, dq, t, tv = (A((B, N), dtype) for _ in range(4))
        u = engine.joint_generate(ARM, N, c, 1, q, dq, dtype=dtype, device=2)
        name, args = fake.last()
        assert name == "abrk_joint_generate_batch" and len(args) == 12
        assert norm(args) == (ARM, CODE[dtype], ref(c), 1, B, addr(q), addr(dq), None, None, addr(u), 2, None)
        assert is_arr(u, KIND[form], (B, N), dtype)
        ug = A((B, N), dtype)
        assert engine.joint_generate(ARM, N, c, [], q, dq, t, tv, ug, dtype, 2, Stream()) is ug
        assert norm(fake.last()[1])[3:] == (0, B, addr(q), addr(dq), addr(t), addr(tv), addr(ug), 2, 0x77)
        with pytest.raises(ValueError, match="target_velocity"):
            engine.joint_generate(ARM, N, c, True, q, dq, t, A((B, 3), dtype), dtype=dtype, device=2)
    q, dq, t, tv = (host((B, N), dtype) for _ in range(4))
    u = engine.joint_generate_sharded(ARM, N, c, True, q, dq, [2, 3, 3], t, tv, dtype)
    name, args = fake.last()
    assert name == "abrk_joint_generate_sharded" and len(args) == 12
    assert norm(args) == (ARM, CODE[dtype], ref(c), 1, B, addr(q), addr(dq), addr(t), addr(tv), addr(u), 3, (2, 3, 3))
    assert is_arr(u, np.ndarray, (B, N), dtype)
    u = engine.joint_generate_sharded(ARM, N, c, False, q, dq, [2], dtype=dtype)
    assert norm(fake.last()[1])[3:] == (0, B, addr(q), addr(dq), None, None, addr(u), 1, (2,))
    with pytest.raises(TypeError, match="target"):
        engine.joint_generate_sharded(ARM, N, c, True, q, dq, [0], dev((B, N), dtype), dtype=dtype)

    devices = [3, 3]
    S = lambda: ShardedArray.empty((4, N), dtype, devices)
    qs, dqs, ts_, tvs, us = S(), S(), S(), S(), S()
    assert engine.joint_generate_resident(ARM, N, c, True, qs, dqs, ts_, tvs, us, dtype, [0x41, 0x42]) is us
    name, args = fake.last()
    assert name == "abrk_joint_generate_resident" and len(args) == 10
    assert norm(args)[:4] == (ARM, CODE[dtype], ref(c), 1) and cut_of(args[4]) == (2, devices, [2, 2], [0x41, 0x42])
    assert norm(args)[5:] == (tab(qs), tab(dqs), tab(ts_), tab(tvs), tab(us))
    u = engine.joint_generate_resident(ARM, N, c, False, qs, dqs, dtype=dtype)
    assert norm(fake.last()[1])[3] == 0 and norm(fake.last()[1])[5:] == (tab(qs), tab(dqs), None, None, tab(u))
    assert type(u) is ShardedArray and u.shape == (4, N) and cut_of(fake.last()[1][4])[3] is None
    with pytest.raises(ValueError, match="target"):
        engine.joint_generate_resident(ARM, N, c, True, qs, dqs, ShardedArray.empty((4, N), dtype, [3, 2]), dtype=dtype)


# ---------------------------------------------------------------------------- the secondary controllers' kernels
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["numpy", "device"])
def test_limits_floating_obstacles_ik(fake, form, dtype):
    A = FORMS[form]
    q, dq, ug = A((B, N), dtype), A((B, N), dtype), A((B, N), dtype)
    lp = _abi.make_limits_params(N, [-1.0] * N, [1.0] * N)
    u = engine.avoid_joint_limits_generate(N, lp, q, None, True, dtype, 2, Stream())
    name, args = fake.last()
    assert name == "abrk_avoid_joint_limits_generate_batch"
    assert norm(args) == (N, CODE[dtype], ref(lp), B, addr(q), addr(u), 0, 2, 0x77) and is_arr(u, KIND[form], (B, N), dtype)
    assert engine.avoid_joint_limits_generate(N, lp, q, ug, True, dtype, 2) is ug
    assert norm(fake.last()[1])[5:] == (addr(ug), 1, 2, None)
    assert engine.avoid_joint_limits_generate(N, lp, q, ug, dtype=dtype, device=2) is ug and fake.last()[1][6] == 0

    u = engine.floating_generate(ARM, N, True, False, q, dq, None, False, dtype, 2, Stream())
    name, args = fake.last()
    assert name == "abrk_floating_generate_batch"
    assert args == (ARM, CODE[dtype], 1, 0, B, addr(q), addr(dq), addr(u), 0, 2, 0x77) and is_arr(u, KIND[form], (B, N), dtype)
    assert engine.floating_generate(ARM, N, False, True, q, dq, ug, True, dtype, 2) is ug
    assert fake.last()[1][2:] == (0, 1, B, addr(q), None, addr(ug), 1, 2, None)

    op = _abi.make_obstacles_params([[0.1, 0.2, 0.3, 0.05]])
    u = engine.avoid_obstacles_generate(ARM, N, op, q, None, False, dtype, 2, Stream())
    name, args = fake.last()
    assert name == "abrk_avoid_obstacles_generate_batch"
    assert norm(args) == (ARM, CODE[dtype], ref(op), B, addr(q), addr(u), 0, 2, 0x77)
    assert engine.avoid_obstacles_generate(ARM, N, op, q, ug, True, dtype, 2) is ug and fake.last()[1][6] == 1
    with pytest.raises(ValueError, match="q"):
        engine.avoid_obstacles_generate(ARM, N, op, A((B, N - 1), dtype), dtype=dtype, device=2)

    ip = _abi.make_ik_params(n_timesteps=11)
    t = A((B, 6), dtype)
    pp, vp = engine.ik_generate_path(ARM, N, ip, q, t, dtype, 2, Stream())
    name, args = fake.last()
    assert name == "abrk_ik_generate_path_batch"
    assert norm(args) == (ARM, CODE[dtype], ref(ip), B, addr(q), addr(t), addr(pp), addr(vp), 2, 0x77)
    assert is_arr(pp, KIND[form], (B, 11, N), dtype) and is_arr(vp, KIND[form], (B, 11, N), dtype)
    g1, g2 = A((B, 11, N), dtype), A((B, 11, N), dtype)
    assert engine.ik_generate_path(ARM, N, ip, q, t, dtype, 2, None, g1, g2) == (g1, g2)
    with pytest.raises(ValueError, match="velocity_path"):
        engine.ik_generate_path(ARM, N, ip, q, t, dtype, 2, None, g1, A((B, 10, N), dtype))


# ---------------------------------------------------------------------------- plants, rollout
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["numpy", "device"])
def test_plants_and_rollout(fake, form, dtype):
    A = FORMS[form]
    other = np.float32 if dtype is np.float64 else np.float64
    tl = _abi.TwoLinkPlant(1.0, 2.0, 3.0, 4.0, 0.001)
    q2, dq2, u2 = A((B, 2), dtype), A((B, 2), dtype), A((B, 2), dtype)
    assert engine.twolink_step(tl, q2, dq2, u2, dtype, 2, Stream()) is None
    name, args = fake.last()
    assert name == "abrk_twolink_step_batch"
    assert norm(args) == (CODE[dtype], ref(tl), B, addr(q2), addr(dq2), addr(u2), 2, 0x77)
    with pytest.raises(ValueError, match="dq"):
        engine.twolink_step(tl, q2, A((B, 2), other), u2, dtype, 2)

    q, dq, u, te, w = (A(s, dtype) for s in ((B, N), (B, N), (B, N), (B, N), (B, 6)))
    ddq = engine.forward_dynamics(ARM, N, q, dq, u, None, dtype, 2, Stream())
    name, args = fake.last()
    assert name == "abrk_forward_dynamics_batch"
    assert args == (ARM, CODE[dtype], B, addr(q), addr(dq), addr(u), addr(ddq), 2, 0x77)
    assert is_arr(ddq, KIND[form], (B, N), dtype)
    fx = _abi.make_plant_effects(N, damping=0.1)
    given = A((B, N), dtype)
    assert engine.forward_dynamics(ARM, N, q, dq, u, given, dtype, 2, None, fx, te, w) is given
    name, args = fake.last()
    assert name == "abrk_forward_dynamics_fx_batch"
    assert norm(args) == (ARM, CODE[dtype], ref(fx), B, addr(q), addr(dq), addr(u), addr(te), addr(w), addr(given), 2, None)
    engine.forward_dynamics(ARM, N, q, dq, u, given, dtype, 2, wrench=w)
    assert norm(fake.last()[1])[2:4] == (None, B) and norm(fake.last()[1])[7:9] == (None, addr(w))
    with pytest.raises(ValueError, match="wrench"):
        engine.forward_dynamics(ARM, N, q, dq, u, None, dtype, 2, wrench=A((B, 5), dtype))

    pl = _abi.make_plant_params(0.001, 2)
    assert engine.plant_step(ARM, N, pl, q, dq, u, dtype, 2, Stream()) is None
    name, args = fake.last()
    assert name == "abrk_plant_step_batch"
    assert norm(args) == (ARM, CODE[dtype], ref(pl), B, addr(q), addr(dq), addr(u), 2, 0x77)
    engine.plant_step(ARM, N, pl, q, dq, u, dtype, 2, None, fx, te)
    name, args = fake.last()
    assert name == "abrk_plant_step_fx_batch"
    assert norm(args) == (ARM, CODE[dtype], ref(pl), ref(fx), B, addr(q), addr(dq), addr(u), addr(te), None, 2, None)
    engine.plant_step(ARM, N, pl, q, dq, u, dtype, 2, tau_ext=te)
    assert norm(fake.last()[1])[3] is None
    if form == "numpy":
        with pytest.raises(ValueError, match="q"):
            engine.plant_step(ARM, N, pl, host((N, B), dtype).T, dq, u, dtype, 2)
        with pytest.raises(TypeError, match="mixing"):
            engine.plant_step(ARM, N, pl, q, dev((B, N), dtype), u, dtype, 2)

    p = _abi.make_osc_params(2, kp=10, ki=0.1)
    t, ie = A((B, 6), dtype), A((B, 6), dtype)
    assert engine.osc_rollout_twolink(ARM, p, tl, q2, dq2, t, 20, dtype=dtype, device=2) is None
    name, args = fake.last()
    assert name == "abrk_osc_rollout_twolink_batch" and len(args) == 16
    assert norm(args) == (ARM, CODE[dtype], ref(p), ref(tl), B, 20, 0, addr(q2), addr(dq2), addr(t), None, None, None,
                          None, 2, None)
    tr = engine.osc_rollout_twolink(ARM, p, tl, q2, dq2, t, 20, 5, ie, True, dtype, 2, Stream())
    assert norm(fake.last()[1])[5:] == (20, 5, addr(q2), addr(dq2), addr(t), addr(ie)) + tuple(addr(x) for x in tr) + (
        2, 0x77)
    assert len(tr) == 3 and all(is_arr(x, KIND[form], (B, 4, 2), dtype) for x in tr)
    with pytest.raises(ValueError, match="integrated_error"):
        engine.osc_rollout_twolink(ARM, p, tl, q2, dq2, t, 20, 5, A((B, 5), dtype), dtype=dtype, device=2)


# ---------------------------------------------------------------------------- path planner entries
@pytest.mark.parametrize("form", ["numpy", "device"])
def test_path_entries(fake, form):
    A = FORMS[form]
    I = (lambda s: np.zeros(s, np.int32)) if form == "numpy" else (lambda s: dev(s, np.int32, 2))
    pp = _abi.PathParams(0.001, 16, 2, 0, 12, 40)
    table, offsets = np.zeros(40), np.arange(10, dtype=np.int64)
    start, target = A((B, 3), np.float64), A((B, 3), np.float64)
    nt, rp, ds = engine.path_plan(pp, table, offsets, start, target, 2, Stream())
    name, args = fake.last()
    assert name == "abrk_path_plan_batch" and len(args) == 11
    assert norm(args) == (ref(pp), addr(table), addr(offsets), B, addr(start), addr(target), addr(nt), addr(rp), addr(ds),
                          2, 0x77)
    assert is_arr(nt, KIND[form], (B,), np.int32) and is_arr(rp, KIND[form], (B, 2), np.int32)
    assert is_arr(ds, KIND[form], (B, 16), np.float64)
    dtab = dev((40,), np.float64, 2)  # the table may live on the device whatever the rows do
    engine.path_plan(pp, dtab, offsets, start, target, 2)
    assert fake.last()[1][1] == dtab.ptr
    with pytest.raises(ValueError, match="offsets"):
        engine.path_plan(pp, table, np.arange(9), start, target, 2)
    with pytest.raises(ValueError, match="table"):
        engine.path_plan(pp, np.zeros(39), offsets, start, target, 2)
    with pytest.raises(ValueError, match="table"):
        engine.path_plan(pp, dev((39,), np.float64, 2), offsets, start, target, 2)

    so, to = A((B, 3), np.float64), A((B, 3), np.float64)
    path = engine.path_fill(pp, table, offsets, 50, start, target, nt, rp, ds, so, to, None, 2, Stream())
    name, args = fake.last()
    assert name == "abrk_path_fill_batch" and len(args) == 15
    assert norm(args) == (ref(pp), addr(table), addr(offsets), B, 50, addr(start), addr(target), addr(so), addr(to),
                          addr(nt), addr(rp), addr(ds), addr(path), 2, 0x77)
    assert is_arr(path, KIND[form], (B, 50, 12), np.float64)
    given = A((B, 50, 12), np.float64)
    assert engine.path_fill(pp, table, offsets, 50, start, target, nt, rp, ds, path=given, device=2) is given
    assert norm(fake.last()[1])[7:9] == (None, None)
    with pytest.raises(ValueError, match="rowplan"):
        engine.path_fill(pp, table, offsets, 50, start, target, nt, I((B, 3)), ds, device=2)
    with pytest.raises(ValueError, match="n_timesteps"):
        engine.path_fill(pp, table, offsets, 50, start, target, A((B,), np.float64), rp, ds, device=2)
    with pytest.raises(TypeError, match="mixing"):
        engine.path_fill(pp, table, offsets, 50, start, target, nt,
                         dev((B, 2), np.int32, 2) if form == "numpy" else np.zeros((B, 2), np.int32), ds, device=2)

    for dtype in DTYPES:
        counter, tg, tvel = I((B,)), A((B, 6), dtype), A((B, 6), dtype)
        assert engine.path_next(path, nt, counter, tg, tvel, dtype, 2, Stream()) is None
        name, args = fake.last()
        assert name == "abrk_path_next_batch"
        assert args == (CODE[dtype], B, 50, 12, addr(path), addr(nt), addr(counter), addr(tg), addr(tvel), 2, 0x77)
        engine.path_next(path, nt, counter, tg, dtype=dtype, device=2)
        assert fake.last()[1][8] is None
        with pytest.raises(ValueError, match="counter"):
            engine.path_next(path, nt, I((B + 1,)), tg, dtype=dtype, device=2)
        with pytest.raises(ValueError, match="target"):
            engine.path_next(path, nt, counter, A((B, 5), dtype), dtype=dtype, device=2)
    with pytest.raises(ValueError, match="path"):
        engine.path_next(A((B, 50, 12), np.float32), nt, I((B,)), A((B, 6), np.float64), device=2)


# ---------------------------------------------------------------------------- loop recorder, adaptive signal
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["numpy", "device"])
def test_loop_trace(fake, form, dtype):
    A = FORMS[form]
    I = (lambda s: np.zeros(s, np.int32)) if form == "numpy" else (lambda s: dev(s, np.int32, 2))
    tp = _abi.make_trace_params(13, every=2, capacity=5, columns=("q", "xyz", "err"))
    q, dq, u, t = A((B, N), dtype), A((B, N), dtype), A((B, N), dtype), A((B, 6), dtype)
    counter, settle, hist, stats = I((B,)), I((B,)), A((5, B, N + 4), dtype), A((B, 4), np.float64)
    assert engine.loop_trace(ARM, N, tp, q, dq, u, t, counter, hist, stats, settle, dtype, 2, Stream()) is None
    name, args = fake.last()
    assert name == "abrk_loop_trace_batch" and len(args) == 14
    assert norm(args) == (ARM, CODE[dtype], ref(tp), B, addr(q), addr(dq), addr(u), addr(t), addr(counter), addr(hist),
                          addr(stats), addr(settle), 2, 0x77)
    engine.loop_trace(ARM, N, tp, None, None, None, t, counter, dtype=dtype, device=2)
    assert norm(fake.last()[1])[3:] == (B, None, None, None, addr(t), addr(counter), None, None, None, 2, None)
    with pytest.raises(ValueError, match="q, dq, u, target"):
        engine.loop_trace(ARM, N, tp, None, None, None, None, counter, dtype=dtype, device=2)
    with pytest.raises(ValueError, match="history"):
        engine.loop_trace(ARM, N, tp, q, dq, u, t, counter, A((5, B, N + 3), dtype), dtype=dtype, device=2)
    with pytest.raises(ValueError, match="settle"):
        engine.loop_trace(ARM, N, tp, q, dq, u, t, counter, settle=A((B,), np.float64), dtype=dtype, device=2)
    for bad in (A((B, 3), np.float64), A((B, 4), np.float32)) + ((host((4, B), np.float64).T,) if form == "numpy" else ()):
        with pytest.raises(ValueError, match="stats"):
            engine.loop_trace(ARM, N, tp, q, dq, u, t, counter, stats=bad, dtype=dtype, device=2)
    mixed = dev((B, 4), np.float64, 2) if form == "numpy" else np.zeros((B, 4))
    with pytest.raises(TypeError, match="mixing"):
        engine.loop_trace(ARM, N, tp, q, dq, u, t, counter, stats=mixed, dtype=dtype, device=2)
    with pytest.raises(TypeError, match="mixing"):
        engine.loop_trace(ARM, N, tp, q, dq, u, t, dev((B,), np.int32) if form == "numpy" else np.zeros(B, np.int32),
                          dtype=dtype, device=2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["numpy", "device"])
def test_adapt_step(fake, form, dtype):
    A = FORMS[form]
    D, O, NN = 4, 2, 10
    ap = _abi.make_adapt_params(D, O, n_neurons=5, n_ensembles=2)
    assert engine.ADAPT_STATE == ("x_f", "e_f", "v", "ref", "a_f", "W", "out_f")
    shapes = engine.adapt_state_shapes(ap, B)
    assert shapes == {"x_f": (B, D), "e_f": (B, O), "v": (B, NN), "ref": (B, NN), "a_f": (B, NN), "W": (B, O, NN),
                      "out_f": (B, O)}
    enc, gain, bias, shift, scale = (A(s, dtype) for s in ((NN, D), (NN,), (NN,), (D,), (D,)))
    in0, in1, tr, uadd = A((B, 3), dtype), A((B, 1), dtype), A((B, O), dtype), A((B, O), dtype)
    state = {k: A(s, dtype) for k, s in shapes.items()}
    out = engine.adapt_step(ap, enc, gain, bias, shift, scale, in0, tr, state, in1, None, uadd, dtype, 2, Stream())
    name, args = fake.last()
    assert name == "abrk_adapt_step_batch" and len(args) == 18
    assert norm(args)[:13] == (CODE[dtype], ref(ap), B, addr(enc), addr(gain), addr(bias), addr(shift), addr(scale),
                               addr(in0), 3, addr(in1), 1, addr(tr))
    st = args[13]._obj
    assert {k: getattr(st, k) for k in engine.ADAPT_STATE} == {k: addr(state[k]) for k in engine.ADAPT_STATE}
    assert norm(args)[14:] == (addr(out), addr(uadd), 2, 0x77) and is_arr(out, KIND[form], (B, O), dtype)
    del state["v"], state["ref"]
    given, in4 = A((B, O), dtype), A((B, D), dtype)
    assert engine.adapt_step(ap, enc, gain, bias, shift, scale, in4, tr, state, out=given, dtype=dtype, device=2) is given
    args = fake.last()[1]
    assert norm(args)[8:12] == (addr(in4), 4, None, 0) and (args[13]._obj.v, args[13]._obj.ref) == (None, None)
    assert args[13]._obj.W == addr(state["W"]) and norm(args)[14:] == (addr(given), None, 2, None)
    with pytest.raises(ValueError, match="gain"):
        engine.adapt_step(ap, enc, A((NN + 1,), dtype), bias, shift, scale, in4, tr, state, dtype=dtype, device=2)
    with pytest.raises(ValueError, match="W"):
        engine.adapt_step(ap, enc, gain, bias, shift, scale, in4, tr, dict(state, W=A((B, NN, O), dtype)), dtype=dtype,
                          device=2)
    with pytest.raises(ValueError, match="u_add"):
        engine.adapt_step(ap, enc, gain, bias, shift, scale, in4, tr, state, u_add=A((B, O + 1), dtype), dtype=dtype,
                          device=2)


# ---------------------------------------------------------------------------- plans
@pytest.mark.parametrize("dtype", DTYPES)
def test_plans(fake, dtype):
    p = _abi.make_osc_params(N, kp=50, ki=0.1)
    q, dq, t, tv, ie, une, u, ts = (dev(s, dtype, 2) for s in ((B, N), (B, N), (B, 6), (B, 6), (B, 6), (B, N), (B, N),
                                                                  (B, N)))
    st = Stream()
    with engine.Plan(2, st) as plan:
        assert fake.last() == ("abrk_plan_begin", (2, 0x77))
        r = engine.osc_generate(ARM, N, p, q, dq, t, tv, ie, une, u, ts, dtype, 2, st)
        u2 = engine.joint_generate(ARM, N, _abi.make_joint(5), True, q, dq, dtype=dtype, device=2, stream=st)
    assert fake.last() == ("abrk_plan_end", ()) and plan.id == 0 and r == (u, ts) and type(u2) is DeviceArray
    rec = [c for c in fake.calls if c[0] in ("abrk_osc_generate_batch", "abrk_joint_generate_batch")]
    assert norm(rec[0][1]) == (ARM, CODE[dtype], ref(p), B) + osc_args(q, dq, t, tv, ie, une, u, ts) + (2, 0x77)
    assert norm(rec[1][1])[9:] == (addr(u2), 2, 0x77)
    plan.launch()
    assert fake.last() == ("abrk_plan_launch", (0,))
    plan.launch_graph(5)
    assert fake.last() == ("abrk_plan_launch_graph", (0, 5))
    plan.launch_repeat(4)
    assert fake.last() == ("abrk_plan_launch_repeat", (0, 4))
    assert plan.keep(q) is plan
    engine.plans_launch([plan, plan], 3, graph=True)
    name, args = fake.last()
    assert name == "abrk_plans_launch" and norm(args) == ((0, 0), 2, 3, 1)
    plan.close()
    assert fake.last() == ("abrk_plan_destroy", (0,)) and plan.id is None
    with pytest.raises(RuntimeError):
        with engine.Plan(2, st):
            raise RuntimeError("x")
    assert fake.last() == ("abrk_plan_abort", ())

    op = engine.OscPlan(ARM, N, p, q, dq, t, u, tv, ie, une, ts, dtype, 2, st)
    name, args = fake.last()
    assert name == "abrk_osc_plan_create" and len(args) == 14 and op.id == 0
    assert norm(args) == (ARM, CODE[dtype], ref(p), B) + osc_args(q, dq, t, tv, ie, une, u, ts) + (2, 0x77)
    assert all(any(k is x for k in op._keep) for x in (q, dq, t, tv, ie, une, u, ts, p, st))
    op2 = engine.OscPlan(ARM, N, p, q, dq, t, u, dtype=dtype, device=2)
    assert norm(fake.last()[1])[4:] == osc_args(q, dq, t, None, None, None, u, None) + (2, None) and op2.id == 0
    n0 = len(fake.named("abrk_osc_plan_create"))
    for k, nm in enumerate(("q", "dq", "target", "u", "target_velocity", "integrated_error", "u_null_ext",
                            "training_signal")):
        a = [q, dq, t, u, tv, ie, une, ts]
        a[k] = np.zeros(a[k].shape, dtype)
        with pytest.raises(TypeError, match=nm):
            engine.OscPlan(ARM, N, p, *a, dtype=dtype, device=2)
    for bad in (np.zeros((B, 5), dtype), np.zeros((B, 6), np.float32 if dtype is np.float64 else np.float64)):
        with pytest.raises(TypeError, match="integrated_error"):
            engine.OscPlan(ARM, N, p, q, dq, t, u, integrated_error=bad, dtype=dtype, device=2)
    with pytest.raises(ValueError, match="target"):
        engine.OscPlan(ARM, N, p, q, dq, dev((B, 5), dtype, 2), u, dtype=dtype, device=2)
    assert len(fake.named("abrk_osc_plan_create")) == n0

    sp = _abi.make_sliding_params(N)
    t3, tv3, ta3, s = dev((B, 3), dtype, 2), dev((B, 3), dtype, 2), dev((B, 3), dtype, 2), dev((B, N), dtype, 2)
    pl = engine.SlidingPlan(ARM, N, sp, q, dq, t3, u, tv3, ta3, s, dtype, 2, st)
    name, args = fake.last()
    assert name == "abrk_sliding_plan_create" and len(args) == 13
    assert norm(args) == (ARM, CODE[dtype], ref(sp), B, addr(q), addr(dq), addr(t3), addr(tv3), addr(ta3), addr(u), addr(s),
                          2, 0x77)
    assert all(any(k is x for k in pl._keep) for x in (q, dq, t3, tv3, ta3, u, s, sp))
    pl2 = engine.SlidingPlan(ARM, N, sp, q, dq, t3, u, dtype=dtype, device=2)
    assert norm(fake.last()[1])[7:] == (None, None, addr(u), None, 2, None) and pl2.id == 0
    for k, nm in enumerate(("q", "dq", "target", "u", "target_velocity", "target_acc", "s")):
        a = [q, dq, t3, u, tv3, ta3, s]
        a[k] = np.zeros(a[k].shape, dtype)
        with pytest.raises(TypeError, match=nm):
            engine.SlidingPlan(ARM, N, sp, *a, dtype=dtype, device=2)
    with pytest.raises(ValueError, match="target"):
        engine.SlidingPlan(ARM, N, sp, q, dq, t, u, dtype=dtype, device=2)

    ml = engine.MergedLoops(ARM, N, p, [2, 3], dtype, 2, st, target_velocity=True, training_signal=True)
    name, args = next(c for c in reversed(fake.calls) if c[0] == "abrk_osc_generate_batch")
    assert norm(args) == (ARM, CODE[dtype], ref(p), 5) + osc_args(ml.q, ml.dq, ml.target, ml.target_velocity,
                                                                 ml.integrated_error, None, ml.u, ml.training_signal) + (2, 0x77)
    v = ml.loop(1)
    assert v.rows == (2, 5) and v.q.shape == (3, N) and v.q.ptr == ml.q.ptr + 2 * N * np.dtype(dtype).itemsize
    assert v.integrated_error.shape == (3, 6) and is_arr(ml.u, DeviceArray, (5, N), dtype)
    ml.launch()
    assert fake.last() == ("abrk_plan_launch", (0,))
    ml.launch_graph(7)
    assert fake.last() == ("abrk_plan_launch_graph", (0, 7))
    ml.close()
    with pytest.raises(ValueError, match="row"):
        engine.MergedLoops(ARM, N, p, [2, 0], dtype, 2, st)


# ---------------------------------------------------------------------------- the controller classes
def ur5_config(dtype=np.float64, **kw):
    from abr_control_amd.arms import ur5

    rc = ur5.Config(dtype=dtype, device=2, **kw)
    rc._arm_id = ARM  # (registering the arm is the library's business)
    return rc


def roles(args, **known):
    """each pointer (or pointer table) argument as the name of the array it belongs to"""
    by = {}
    for k, v in known.items():
        if v is not None:
            by[tab(v) if isinstance(v, ShardedArray) else addr(v)] = k
    return tuple(None if a is None else by.get(a, "?") for a in norm(args))


def make_ctrlr(kind, rc):
    from abr_control_amd import controllers as cc

    if kind == "OSC":
        return cc.OSC(rc, kp=50, kv=7, ki=0.1, use_C=True, null_controllers=[cc.Damping(rc, 3), cc.RestingConfig(
            rc, [None, 1.0, 2.0, None, 0.5, None], kp=4, kv=2)])
    if kind == "Sliding":
        return cc.Sliding(rc, kd=120.0, lamb=25.0)
    if kind == "Joint":
        return cc.Joint(rc, kp=20, kv=4)
    if kind == "Damping":
        return cc.Damping(rc, kv=7)
    return cc.RestingConfig(rc, [None, 0.8, -1.6, None, 1.5, None], kp=30, kv=6)


STEM = {"OSC": "abrk_osc_generate", "Sliding": "abrk_sliding_generate", "Joint": "abrk_joint_generate",
        "Damping": "abrk_joint_generate", "RestingConfig": "abrk_joint_generate"}
# the arrays of each call in the order of the C signature, None where the controller passes NULL
ROLES = {"OSC": ("q", "dq", "target", "target_velocity", "integrated_error", None, "u", "training_signal"),
         "Sliding": ("q", "dq", "target", "target_velocity", None, "u", "s"),
         "Joint": ("q", "dq", "target", "target_velocity", "u"),
         "Damping": ("q", "dq", None, None, "u"), "RestingConfig": ("q", "dq", None, None, "u")}
N_HEAD = {"OSC": 4, "Sliding": 4, "Joint": 5, "Damping": 5, "RestingConfig": 5}
OUTPUTS = {"OSC": ("training_signal", "integrated_error"), "Sliding": ("s",), "Joint": (), "Damping": (),
           "RestingConfig": ()}


def ctrl_inputs(kind, nb, dtype):
    rs = np.random.RandomState(5)
    sh = (N,) if nb == 0 else (nb, N)
    q, dq = rs.uniform(0, 1, sh).astype(dtype), rs.uniform(0, 1, sh).astype(dtype)
    tw = {"OSC": 6, "Sliding": 3, "Joint": N}.get(kind)
    if tw is None:
        return (q, dq), ("q", "dq")
    tsh = (tw,) if nb == 0 else (nb, tw)
    return (q, dq, rs.uniform(0, 1, tsh).astype(dtype), rs.uniform(0, 1, tsh).astype(dtype)), (
        "q", "dq", "target", "target_velocity")


def head_of(kind, args):
    """the by-value part in front of the arrays: struct bytes and scalars, without the row count / cut"""
    h = [bytes(a._obj) if hasattr(a, "_obj") else a for a in args[:N_HEAD[kind]]]
    return h[:-1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", [0, 1, B])
@pytest.mark.parametrize("kind", list(STEM))
def test_multidevice_host_batch_sends_what_the_controller_sends(fake, kind, nb, dtype):
    rc = ur5_config(dtype, reference_dtypes=False)
    md = MultiDevice([0, 1, 1])
    arrays, names = ctrl_inputs(kind, nb, dtype)
    known = dict(zip(names, arrays))
    sent = {}
    for via in ("ctrlr", "md"):
        c = make_ctrlr(kind, rc)
        u = c.generate(*arrays) if via == "ctrlr" else md.generate(c, *arrays)
        name, args = fake.last(STEM[kind])
        outs = {k: getattr(c, k) for k in OUTPUTS[kind]}
        nh = N_HEAD[kind]
        ptrs = args[nh:nh + len(ROLES[kind])]
        assert roles(ptrs, u=u, **known, **outs) == ROLES[kind], via
        sent[via] = (head_of(kind, args), args[nh - 1])
        assert name == STEM[kind] + ("_batch" if via == "ctrlr" else "_sharded")
        assert norm(args)[nh + len(ROLES[kind]):] == ((2, None) if via == "ctrlr" else (3, (0, 1, 1)))
        shape = (N,) if nb == 0 else (nb, N)
        assert is_arr(u, np.ndarray, shape, dtype)
        for k, v in outs.items():
            assert is_arr(v, np.ndarray, (6,) if (k == "integrated_error" and nb == 0) else
                          (nb, 6) if k == "integrated_error" else shape, dtype), k
    assert sent["ctrlr"] == sent["md"] and sent["md"][1] == max(nb, 1)
    head = sent["md"][0]
    assert head[:2] == [ARM, CODE[dtype]]
    if kind == "OSC":
        p = _abi.OSCParams.from_buffer_copy(head[2])
        assert (p.kp, p.ko, p.kv, p.ki, p.use_C, p.use_g, p.n_null, p.ref_frame) == (50, 50, 7, 0.1, 1, 1, 2, 13)
        assert (p.null_ctrl[0].kv, p.null_ctrl[1].kp, list(p.null_ctrl[1].rest_mask)[:N]) == (3, 4, [0, 1, 1, 0, 1, 0])
    elif kind == "Sliding":
        p = _abi.SlidingParams.from_buffer_copy(head[2])
        assert (p.kd, p.lamb, p.cartesian, p.ref_frame, list(p.offset)) == (120.0, 25.0, 1, 13, [0, 0, 0])
    else:
        p = _abi.NullCtrl.from_buffer_copy(head[2])
        assert (p.kp, p.kv) == {"Joint": (20, 4), "Damping": (0, 7), "RestingConfig": (30, 6)}[kind]
        assert head[3] == (1 if kind == "Joint" else 0)
        assert bytes(p) == bytes({"Joint": _abi.make_joint(20, 4), "Damping": _abi.make_damping(7),
                                  "RestingConfig": _abi.make_resting([None, 0.8, -1.6, None, 1.5, None], 30, 6)}[kind])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", list(STEM))
def test_multidevice_resident_sends_what_the_controller_sends(fake, kind, dtype):
    rc = ur5_config(dtype, reference_dtypes=False)
    md = MultiDevice([0, 1, 1])
    arrays, names = ctrl_inputs(kind, 5, dtype)
    c = make_ctrlr(kind, rc)
    c.generate(*arrays)
    name, args = fake.last(STEM[kind])
    direct = head_of(kind, args)
    sharded = [md.scatter(a) for a in arrays]
    c = make_ctrlr(kind, rc)
    u = md.generate(c, *sharded)
    name, args = fake.last(STEM[kind])
    nh = N_HEAD[kind]
    assert name == STEM[kind] + "_resident" and len(args) == nh + len(ROLES[kind])
    assert head_of(kind, args) == direct
    assert cut_of(args[nh - 1]) == (3, [0, 1, 1], [2, 2, 1], [0x5000, 0x5100, 0x5101])
    outs = {k: getattr(c, k) for k in OUTPUTS[kind]}
    assert roles(args[nh:], u=u, **dict(zip(names, sharded)), **outs) == ROLES[kind]
    assert type(u) is ShardedArray and u.shape == (5, N) and u.dtype == np.dtype(dtype) and u.devices == [0, 1, 1]
    for k, v in outs.items():
        assert type(v) is ShardedArray and v.shape == (5, 6 if k == "integrated_error" else N) and v.rows == [2, 2, 1]
    if kind == "OSC":  # the state stays with its shards from one tick to the next; it starts from zero
        ie = c.integrated_error
        assert len(fake.named("abrk_memset")) == 3
        md.generate(c, *sharded)
        assert c.integrated_error is ie and norm(fake.last(STEM[kind])[1])[nh + 4] == tab(ie)
    with pytest.raises(ValueError, match="devices"):
        MultiDevice([0, 1, 2]).generate(c, *sharded)
    if kind == "Sliding":
        md.generate(c, sharded[0], sharded[1], sharded[2], None, target_acc=None)
        assert norm(fake.last(STEM[kind])[1])[nh + 3:nh + 5] == (None, None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_controllers_on_device_arrays_and_reference_dtypes(fake, dtype):
    from abr_control_amd import controllers as cc

    rc = ur5_config(dtype)
    q, dq, t = dev((B, N), dtype, 2), dev((B, N), dtype, 2), dev((B, 6), dtype, 2)
    c = cc.OSC(rc, kp=50, ki=0.1)
    u = c.generate(q, dq, t)
    args = fake.last("abrk_osc_generate")[1]
    assert roles(args[4:12], q=q, dq=dq, target=t, u=u, training_signal=c.training_signal,
                 integrated_error=c.integrated_error) == ("q", "dq", "target", None, "integrated_error", None, "u",
                                                          "training_signal")
    assert is_arr(u, DeviceArray, (B, N), dtype) and is_arr(c.integrated_error, DeviceArray, (B, 6), dtype)
    u, dyn = c.generate(q, dq, t, return_dynamics=("J", "M"))
    name, args = fake.last("abrk_osc_generate")
    assert name == "abrk_osc_generate_full_batch" and args[12] == 6 and dyn_out(args[13]._obj, dyn)
    sl = cc.Sliding(rc)
    t3 = dev((B, 3), dtype, 2)
    u = sl.generate(q, dq, t3, 0, t3)
    assert roles(fake.last("abrk_sliding")[1][4:11], q=q, dq=dq, target=t3, u=u, s=sl.s) == (
        "q", "dq", "target", None, "target", "u", "s")
    assert type(cc.Joint(rc).generate(q, dq, q)) is DeviceArray and type(cc.Damping(rc, 2).generate(q, dq)) is DeviceArray
    # NumPy in: the reference's float64 out, whatever the kernel computes in; scalars as the reference takes them
    qh, dqh, th = host((B, N), dtype), host((B, N), dtype), host((B, 6), dtype)
    c = cc.OSC(rc, kp=50, ki=0.1)
    u = c.generate(qh, dqh, th)
    assert is_arr(u, np.ndarray, (B, N), np.float64) and is_arr(c.training_signal, np.ndarray, (B, N), np.float64)
    assert is_arr(c.integrated_error, np.ndarray, (B, 6), dtype)
    u, dyn = c.generate(qh[0], dqh[0], th[0], return_dynamics=("Tx",))
    assert u.shape == (N,) and dyn["Tx"].shape == (3,) and c.integrated_error.shape == (6,)
    u = sl.generate(qh, dqh, th[:, :3], 0.5)
    args = fake.last("abrk_sliding")[1]
    assert args[7] is not None and args[8] is None and is_arr(sl.s, np.ndarray, (B, N), np.float64)
    for k in (cc.Joint(rc).generate(qh, dqh, qh), cc.Damping(rc, 2).generate(qh[0], dqh[0]),
              cc.RestingConfig(rc, [0.1] * N).generate(qh, dqh)):
        assert k.dtype == np.float64
    # more Damping / RestingConfig than the kernel fuses: the rest is summed into u_null_ext
    extra = [cc.Damping(rc, k + 1) for k in range(5)]
    c5 = cc.OSC(rc, kp=50, null_controllers=extra + [cc.Joint(rc)])
    assert c5._fused_src == extra[:4] and c5._device == extra[4:] and len(c5._foreign) == 1
    assert [hasattr(x, "_accumulate") for x in (cc.Damping, cc.RestingConfig, cc.Joint, cc.Sliding, cc.Controller, cc.OSC,
                                                cc.AvoidJointLimits, cc.AvoidObstacles, cc.Floating)] == [
        True, True, False, False, False, False, True, True, True]
    une = np.zeros((B, N), dtype)
    extra[4]._accumulate(qh, dqh, une)
    name, args = fake.last()
    assert name == "abrk_joint_generate_batch" and bytes(args[2]._obj) == bytes(_abi.make_damping(5))
    assert args[3:7] == (0, B, addr(qh), addr(dqh)) and args[7:9] == (None, None) and args[10:] == (2, None)
    cc.RestingConfig(rc, [0.1] * N, kp=3)._accumulate(qh, dqh, une)
    assert bytes(fake.last()[1][2]._obj) == bytes(_abi.make_resting([0.1] * N, 3))
    with pytest.raises(TypeError, match="null controllers"):
        extra[4]._accumulate(q, dq, dev((B, N), dtype, 2))


def test_multidevice_refusals_and_streams(fake):
    from abr_control_amd import controllers as cc

    rc = ur5_config()
    md = MultiDevice([0, 1, 1, 0])
    assert [(s.device, s.ptr) for s in md.streams] == [(0, 0x5000), (1, 0x5100), (1, 0x5101), (0, 0x5001)]
    qs = md.scatter(np.zeros((6, N)))
    n0 = len(fake.calls)
    qs.numpy()
    got = [(c[1][0], c[1][4]) for c in fake.calls[n0:] if c[0] == "abrk_memcpy_d2h"]
    assert got == [(0, 0x5000), (1, 0x5100), (1, 0x5101), (0, 0x5001)]  # each shard is gathered on its own stream
    md.sync()
    name, args = fake.last()
    assert name == "abrk_shards_sync" and cut_of(args[0]) == (4, [0, 1, 1, 0], [1, 1, 1, 1],
                                                              [0x5000, 0x5100, 0x5101, 0x5001])
    q, dq, t = np.zeros((B, N)), np.zeros((B, N)), np.zeros((B, 6))
    for bad in (cc.OSC(rc, null_controllers=[cc.Floating(rc)]), cc.OSC(rc, null_controllers=[cc.Controller(rc)])):
        with pytest.raises(TypeError, match="fused null controllers"):
            md.generate(bad, q, dq, t)
        with pytest.raises(TypeError, match="fused null controllers"):
            md.generate(bad, md.scatter(q), md.scatter(dq), md.scatter(t))
        with pytest.raises(TypeError, match="fused null controllers"):
            md.record_generate(bad, md.scatter(q), md.scatter(dq), md.scatter(t))
    with pytest.raises(TypeError, match="fused null controllers"):
        md.record_generate(cc.Sliding(rc), md.scatter(q), md.scatter(dq), md.scatter(t))
    for c in (cc.Floating(rc), cc.AvoidJointLimits(rc, [-1] * N, [1] * N)):
        with pytest.raises(TypeError, match=type(c).__name__):
            md.generate(c, q, dq)
        with pytest.raises(TypeError, match=type(c).__name__):
            md.generate(c, md.scatter(q), md.scatter(dq))
    for c, a in ((cc.OSC(rc), (t,)), (cc.Sliding(rc), (t[:, :3],)), (cc.Damping(rc, 1), ())):
        with pytest.raises(TypeError, match="NumPy"):
            md.generate(c, dev((B, N), np.float64), dq, *a)
    with pytest.raises(ValueError, match="devices"):
        MultiDevice([0, 9])

    # a recorded tick per shard
    md = MultiDevice([0, 1])
    c = cc.OSC(rc, kp=50, ki=0.1)
    qs, dqs, ts_ = md.scatter(q), md.scatter(dq), md.scatter(t)
    n0 = len(fake.calls)
    plan = md.record_generate(c, qs, dqs, ts_)
    rec = [x for x in fake.calls[n0:] if x[0] in ("abrk_plan_begin", "abrk_osc_generate_batch", "abrk_plan_end")]
    assert [x[0] for x in rec] == ["abrk_plan_begin", "abrk_osc_generate_batch", "abrk_plan_end"] * 2
    assert rec[0][1] == (0, 0x5000) and rec[3][1] == (1, 0x5100)
    ie, tsg = c.integrated_error, c.training_signal
    for g in range(2):
        assert norm(rec[1 + 3 * g][1])[3:] == (qs.rows[g],) + tuple(x.parts[g].ptr for x in (qs, dqs, ts_)) + (
            None, ie.parts[g].ptr, None, plan.u.parts[g].ptr, tsg.parts[g].ptr, g, 0x5000 + 0x100 * g)
    assert plan.training_signal is tsg and type(plan.u) is ShardedArray
    plan.launch(3)
    assert norm(fake.last()[1]) == ((0, 0), 2, 3, 0)
    plan.sync()
    assert cut_of(fake.last()[1][0])[3] == [0x5000, 0x5100]
    plan.close()


@pytest.mark.parametrize("kind", list(STEM))
@pytest.mark.parametrize("resident", [False, True])
def test_multidevice_keeps_no_routing_state_on_the_controller(fake, kind, resident):
    """a controller shared by two threads must not send one thread's plain generate() over the other's devices: where
    a call runs is an argument of the call, never an attribute of the controller"""
    rc = ur5_config()
    md = MultiDevice([0, 1, 1])
    arrays, _ = ctrl_inputs(kind, 5, np.float64)
    if resident:
        arrays = [md.scatter(a) for a in arrays]
    c = make_ctrlr(kind, rc)
    before = set(vars(c))
    seen = []
    fake.hook = lambda name, args: seen.append(set(vars(c))) if name.startswith(STEM[kind]) else None
    md.generate(c, *arrays)
    fake.hook = None
    assert seen == [before]
    assert set(vars(c)) == before
    assert not hasattr(c, "_shard_devices") and not hasattr(type(c), "_shard_devices")
    for k in OUTPUTS[kind]:
        assert getattr(c, k) is not None


# ---------------------------------------------------------------------------- the public surface
SIGNATURES = {
    "engine.dynamics": "(arm_id, n, q, dq=None, frame=None, x_off=None, want=('M',), dtype=<class 'numpy.float64'>, device=0, stream=None, out=None)",
    "engine.osc_generate": "(arm_id, n, params, q, dq, target, target_velocity=None, integrated_error=None, u_null_ext=None, u=None, training_signal=False, dtype=<class 'numpy.float64'>, device=0, stream=None, want=None, out=None)",
    "engine.osc_generate_coop": "(arm_id, n, params, q, dq, target, lanes_per_arm, u=None, training_signal=False, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.osc_generate_sharded": "(arm_id, n, params, q, dq, target, devices, target_velocity=None, integrated_error=None, u_null_ext=None, u=None, training_signal=False, dtype=<class 'numpy.float64'>)",
    "engine.sliding_generate_sharded": "(arm_id, n, params, q, dq, target, devices, target_velocity=None, target_acc=None, want_s=False, dtype=<class 'numpy.float64'>)",
    "engine.joint_generate_sharded": "(arm_id, n, ctrl, account_for_gravity, q, dq, devices, target=None, target_velocity=None, dtype=<class 'numpy.float64'>)",
    "engine.dynamics_sharded": "(arm_id, n, q, devices, dq=None, frame=None, x_off=None, want=('M',), dtype=<class 'numpy.float64'>)",
    "engine.osc_generate_resident": "(arm_id, n, params, q, dq, target, target_velocity=None, integrated_error=None, u_null_ext=None, u=None, training_signal=False, dtype=<class 'numpy.float64'>, streams=None)",
    "engine.sliding_generate_resident": "(arm_id, n, params, q, dq, target, target_velocity=None, target_acc=None, u=None, want_s=False, dtype=<class 'numpy.float64'>, streams=None)",
    "engine.joint_generate_resident": "(arm_id, n, ctrl, account_for_gravity, q, dq, target=None, target_velocity=None, u=None, dtype=<class 'numpy.float64'>, streams=None)",
    "engine.dynamics_resident": "(arm_id, n, q, dq=None, frame=None, x_off=None, want=('M',), dtype=<class 'numpy.float64'>, streams=None, out=None)",
    "engine.shards_sync": "(like, streams=None)",
    "engine.plans_launch": "(plans, repeat=1, graph=False)",
    "engine.osc_law": "(n, params, J, M, dq, target, g=None, Cdq=None, xyz=None, R=None, q=None, target_velocity=None, integrated_error=None, u_null_ext=None, training_signal=False, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.osc_mx": "(n, M, J, threshold=0.001, want_minv=True, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.osc_velocity_limiting": "(params, u_task, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.osc_orientation_forces": "(algorithm, R, target_abg, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.transformations": "(op, a, b=None, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.sliding_generate": "(arm_id, n, params, q, dq, target, target_velocity=None, target_acc=None, u=None, want_s=False, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.joint_generate": "(arm_id, n, ctrl, account_for_gravity, q, dq, target=None, target_velocity=None, u=None, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.avoid_joint_limits_generate": "(n, params, q, u=None, accumulate=False, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.floating_generate": "(arm_id, n, dynamic, task_space, q, dq=None, u=None, accumulate=False, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.avoid_obstacles_generate": "(arm_id, n, params, q, u=None, accumulate=False, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.twolink_step": "(plant, q, dq, u, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.forward_dynamics": "(arm_id, n, q, dq, u, ddq=None, dtype=<class 'numpy.float64'>, device=0, stream=None, effects=None, tau_ext=None, wrench=None)",
    "engine.plant_step": "(arm_id, n, params, q, dq, u, dtype=<class 'numpy.float64'>, device=0, stream=None, effects=None, tau_ext=None, wrench=None)",
    "engine.osc_rollout_twolink": "(arm_id, params, plant, q, dq, target, n_steps, every=0, integrated_error=None, want_traj=False, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.path_plan": "(params, table, offsets, start, target, device=0, stream=None)",
    "engine.path_fill": "(params, table, offsets, t_max, start, target, n_timesteps, rowplan, dist_steps, start_orientation=None, target_orientation=None, path=None, device=0, stream=None)",
    "engine.path_next": "(path, n_timesteps, counter, target, target_velocity=None, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.loop_trace": "(arm_id, n, params, q, dq, u, target, counter, history=None, stats=None, settle=None, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.adapt_state_shapes": "(params, B)",
    "engine.adapt_step": "(params, enc, gain, bias, shift, scale, in0, training, state, in1=None, out=None, u_add=None, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.Plan.__init__": "(self, device=0, stream=None)",
    "engine.Plan.keep": "(self, *objs)",
    "engine.Plan.launch": "(self)",
    "engine.Plan.launch_graph": "(self, repeat)",
    "engine.Plan.launch_repeat": "(self, repeat)",
    "engine.Plan.close": "(self)",
    "engine.OscPlan.__init__": "(self, arm_id, n, params, q, dq, target, u, target_velocity=None, integrated_error=None, u_null_ext=None, training_signal=None, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.SlidingPlan.__init__": "(self, arm_id, n, params, q, dq, target, u, target_velocity=None, target_acc=None, s=None, dtype=<class 'numpy.float64'>, device=0, stream=None)",
    "engine.MergedLoops.__init__": "(self, arm_id, n, params, rows_per_loop, dtype=<class 'numpy.float64'>, device=0, stream=None, target_velocity=False, training_signal=False)",
    "engine.MergedLoops.loop": "(self, i)",
    "engine.MergedLoops.launch": "(self)",
    "engine.MergedLoops.launch_graph": "(self, repeat)",
    "engine.MergedLoops.close": "(self)",
    "engine.ik_generate_path": "(arm_id, n, params, position, target, dtype=<class 'numpy.float64'>, device=0, stream=None, position_path=None, velocity_path=None)",
    "sharding.dist_env": "()",
    "sharding.HostGroup.__init__": "(self, rank, world, timeout=120.0, key=None)",
    "sharding.HostGroup.exchange": "(self, value=None)",
    "sharding.HostGroup.barrier": "(self)",
    "sharding.HostGroup.max": "(self, x)",
    "sharding.HostGroup.close": "(self)",
    "sharding.shard_range": "(B, rank, world)",
    "sharding.shard_rows": "(arrays, rank, world)",
    "sharding.ShardedArray.__init__": "(self, parts, devices)",
    "sharding.ShardedArray.cut": "(B, G)",
    "sharding.ShardedArray.empty": "(shape, dtype, devices, rows=None)",
    "sharding.ShardedArray.zeros": "(shape, dtype, devices, rows=None)",
    "sharding.ShardedArray.from_numpy": "(a, devices, dtype=None)",
    "sharding.ShardedArray.numpy": "(self, streams=None)",
    "sharding.ShardedArray.copy_from_numpy": "(self, a)",
    "sharding.ShardedPlan.__init__": "(self, plans, streams, like, results)",
    "sharding.ShardedPlan.launch": "(self, repeat=1)",
    "sharding.ShardedPlan.launch_graph": "(self, repeat)",
    "sharding.ShardedPlan.sync": "(self)",
    "sharding.ShardedPlan.close": "(self)",
    "sharding.MultiDevice.__init__": "(self, devices=None)",
    "sharding.MultiDevice.scatter": "(self, a, dtype=None)",
    "sharding.MultiDevice.empty": "(self, shape, dtype)",
    "sharding.MultiDevice.zeros": "(self, shape, dtype)",
    "sharding.MultiDevice.sync": "(self, like=None)",
    "sharding.MultiDevice.record": "(self, fn)",
    "sharding.MultiDevice.record_generate": "(self, ctrlr, q, dq, target, target_velocity=None, ref_frame='EE', xyz_offset=None, u=None, training_signal=True)",
    "sharding.MultiDevice.generate": "(self, ctrlr, q, dq, *args, **kwargs)",
    "sharding.MultiDevice.dynamics": "(self, robot_config, q, dq=None, name='EE', x=None, want=('Tx', 'J', 'M', 'g'))",
    "controllers.AvoidJointLimits.__init__": "(self, robot_config, min_joint_angles, max_joint_angles, max_torque=None, cross_zero=None, gradient=None)",
    "controllers.AvoidJointLimits.generate": "(self, q, dq=None)",
    "controllers.AvoidObstacles.__init__": "(self, robot_config, obstacles=None, threshold=0.2, gain=1, maximum=500)",
    "controllers.AvoidObstacles.set_obstacles": "(self, obstacles)",
    "controllers.AvoidObstacles.generate": "(self, q, dq=None)",
    "controllers.Controller.__init__": "(self, robot_config)",
    "controllers.Controller.generate": "(self, q, dq)",
    "controllers.Damping.__init__": "(self, robot_config, kv)",
    "controllers.Damping.generate": "(self, q, dq)",
    "controllers.Floating.__init__": "(self, robot_config, dynamic=False, task_space=False)",
    "controllers.Floating.generate": "(self, q, dq=None)",
    "controllers.Joint.__init__": "(self, robot_config, kp=1, kv=None, quaternions=None, account_for_gravity=True)",
    "controllers.Joint.q_tilde_angle": "(self, q, target)",
    "controllers.Joint.generate": "(self, q, dq, target, target_velocity=None)",
    "controllers.OSC.__init__": "(self, robot_config, kp=1, ko=None, kv=None, ki=0, vmax=None, ctrlr_dof=None, null_controllers=None, use_g=True, use_C=False, orientation_algorithm=0)",
    "controllers.OSC.generate": "(self, q, dq, target, target_velocity=None, ref_frame='EE', xyz_offset=None, return_dynamics=None)",
    "controllers.RestingConfig.__init__": "(self, robot_config, rest_angles, **kwargs)",
    "controllers.RestingConfig.q_tilde_angle": "(self, q, target=None)",
    "controllers.RestingConfig.generate": "(self, q, dq)",
    "controllers.Sliding.__init__": "(self, robot_config, kd=160.0, lamb=30.0, cartesian=True)",
    "controllers.Sliding.generate": "(self, q, dq, target, target_velocity=0, target_acc=0, ref_frame='EE', offset=None)",
}


def test_public_signatures():
    """bench.py and the GPU tests call these positionally: names, order and defaults stay"""
    from abr_control_amd import controllers

    mods = {"engine": engine, "sharding": sharding, "controllers": controllers}
    for path, expected in SIGNATURES.items():
        obj = mods[path.split(".")[0]]
        for part in path.split(".")[1:]:
            obj = getattr(obj, part)
        assert str(inspect.signature(obj)) == expected, path
    # ... and nothing public that the table does not name
    for modname in ("engine", "sharding"):
        mod = mods[modname]
        for k, v in vars(mod).items():
            if k.startswith("_") or getattr(v, "__module__", None) != mod.__name__:
                continue
            if inspect.isfunction(v):
                assert f"{modname}.{k}" in SIGNATURES, k
            elif inspect.isclass(v):
                for m in dir(v):
                    if not m.startswith("_") and inspect.isroutine(getattr(v, m)):
                        assert any(f"{modname}.{b.__name__}.{m}" in SIGNATURES for b in v.__mro__), (k, m)
