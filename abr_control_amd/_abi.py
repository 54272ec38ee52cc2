"""ctypes mirror of include/abrk.h (plain data only) + arm-table helpers.

Kept free of any device code so that tools and tests can build `abrk_arm_desc` /
`abrk_osc_params` values without touching the GPU library.
"""
import ctypes as C
import json
import os

import numpy as np

MAX_JOINTS = 7
MAX_NULL = 4

F64, F32 = 0, 1
NULL_DAMPING, NULL_RESTING = 1, 2

WANT_TX = 1 << 0
WANT_J = 1 << 1
WANT_M = 1 << 2
WANT_G = 1 << 3
WANT_C = 1 << 4
WANT_DJ = 1 << 5
WANT_R = 1 << 6
WANT_T = 1 << 7
WANT_TINV = 1 << 8
WANT_QUAT = 1 << 9

ERRORS = {-1: "EINVAL", -2: "ENODEV", -3: "ENOMEM", -4: "ENOARM", -5: "EFRAME", -6: "ESINGULAR", -7: "EPATH"}
ESINGULAR = -6
EPATH = -7


class ArmDesc(C.Structure):
    _fields_ = [
        ("n_joints", C.c_int32),
        ("n_links_dyn", C.c_int32),
        ("has_ee", C.c_int32),
        ("reserved", C.c_int32),
        ("A0", C.c_double * 12),
        ("AJ", (C.c_double * 12) * MAX_JOINTS),
        ("B", (C.c_double * 12) * MAX_JOINTS),
        ("E", C.c_double * 12),
        ("mdiag", (C.c_double * 6) * (MAX_JOINTS + 1)),
        ("name", C.c_char * 32),
    ]


class ArmInertia(C.Structure):  # abrk_arm_inertia: full link / joint inertias of a general-inertia arm
    _fields_ = [
        ("mlink", (C.c_double * 36) * (MAX_JOINTS + 1)),
        ("mjoint", (C.c_double * 36) * MAX_JOINTS),
    ]


class DynOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("Tx", "J", "M", "g", "C", "dJ", "R", "T", "Tinv", "quat")]


class ScratchInfo(C.Structure):  # abrk_scratch_info
    _fields_ = [(k, C.c_int64) for k in ("worklist_slots", "worklist_bytes", "inline_fallbacks", "evictions",
                                          "device_free_bytes", "device_total_bytes", "status_words_out",
                                          "status_blocks")]


class ShardCut(C.Structure):  # abrk_shard_cut: how a resident batch is cut over the devices
    _fields_ = [("n_shards", C.c_int32), ("devices", C.POINTER(C.c_int32)), ("rows", C.POINTER(C.c_int64)),
                ("streams", C.POINTER(C.c_void_p))]


class NullCtrl(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("rest_mask", C.c_int32 * MAX_JOINTS),
        ("kp", C.c_double),
        ("kv", C.c_double),
        ("rest_angles", C.c_double * MAX_JOINTS),
    ]


class OSCParams(C.Structure):
    _fields_ = [
        ("kp", C.c_double),
        ("ko", C.c_double),
        ("kv", C.c_double),
        ("ki", C.c_double),
        ("use_vmax", C.c_int32),
        ("use_g", C.c_int32),
        ("use_C", C.c_int32),
        ("orientation_algorithm", C.c_int32),
        ("vmax", C.c_double * 2),
        ("ctrlr_dof", C.c_int32 * 6),
        ("ref_frame", C.c_int32),
        ("n_null", C.c_int32),
        ("xyz_offset", C.c_double * 3),
        ("null_ctrl", NullCtrl * MAX_NULL),
    ]


class SlidingParams(C.Structure):
    _fields_ = [
        ("kd", C.c_double),
        ("lamb", C.c_double),
        ("cartesian", C.c_int32),
        ("ref_frame", C.c_int32),
        ("offset", C.c_double * 3),
    ]


class IkParams(C.Structure):
    _fields_ = [("max_dx", C.c_double), ("max_dr", C.c_double), ("max_dq", C.c_double), ("dt", C.c_double),
                ("n_timesteps", C.c_int32), ("method", C.c_int32)]


def make_ik_params(max_dx=0.2, max_dr=2 * np.pi, max_dq=np.pi, n_timesteps=200, dt=0.001, method=3):
    """InverseKinematics(max_dx, max_dr, max_dq).generate_path(n_timesteps, dt, method) defaults
    (controllers/path_planners/inverse_kinematics.py:21-37)."""
    p = IkParams()
    p.max_dx, p.max_dr, p.max_dq, p.dt = max_dx, max_dr, max_dq, dt
    p.n_timesteps, p.method = int(n_timesteps), int(method)
    return p


MAX_OBSTACLES = 16


class LimitsParams(C.Structure):
    _fields_ = [
        ("min_joint_angles", C.c_double * MAX_JOINTS),
        ("max_joint_angles", C.c_double * MAX_JOINTS),
        ("max_torque", C.c_double * MAX_JOINTS),
        ("cross_zero", C.c_int32 * MAX_JOINTS),
        ("gradient", C.c_int32 * MAX_JOINTS),
        ("no_limits_min", C.c_int32 * MAX_JOINTS),
        ("no_limits_max", C.c_int32 * MAX_JOINTS),
    ]


class ObstaclesParams(C.Structure):
    _fields_ = [
        ("n_obstacles", C.c_int32),
        ("reserved", C.c_int32),
        ("threshold", C.c_double),
        ("gain", C.c_double),
        ("maximum", C.c_double),
        ("obstacles", (C.c_double * 4) * MAX_OBSTACLES),
    ]


def make_limits_params(n_joints, min_joint_angles, max_joint_angles, max_torque=None, cross_zero=None,
                       gradient=None):
    """AvoidJointLimits.__init__ (avoid_joint_limits.py:35-81) -> abrk_limits_params: limits shifted by
    -pi (:45-50), swapped where cross_zero (:62-66), 'no limit' = NaN (or None) flagged (:74-75)."""
    n = int(n_joints)
    mn = np.array([np.nan if v is None else float(v) for v in min_joint_angles], dtype=float) - np.pi
    mx = np.array([np.nan if v is None else float(v) for v in max_joint_angles], dtype=float) - np.pi
    if mn.shape[0] != n or mx.shape[0] != n:
        raise Exception("joint angles vector incorrect size")  # avoid_joint_limits.py:68-72
    cz = np.zeros(n, bool) if cross_zero is None else np.array(cross_zero, dtype=bool)
    gr = np.zeros(n, bool) if gradient is None else np.array(gradient, dtype=bool)
    tmin, tmax = mn.copy(), mx.copy()
    mx[cz], mn[cz] = tmin[cz], tmax[cz]
    mt = np.ones(n) if max_torque is None else np.asarray(max_torque, dtype=float)
    p = LimitsParams()
    for i in range(n):
        p.no_limits_min[i], p.no_limits_max[i] = int(np.isnan(mn[i])), int(np.isnan(mx[i]))
        p.min_joint_angles[i] = 0.0 if np.isnan(mn[i]) else mn[i]
        p.max_joint_angles[i] = 0.0 if np.isnan(mx[i]) else mx[i]
        p.max_torque[i] = mt[i]
        p.cross_zero[i], p.gradient[i] = int(cz[i]), int(gr[i])
    return p


def make_obstacles_params(obstacles=None, threshold=0.2, gain=1, maximum=500):
    """AvoidObstacles.__init__ / set_obstacles (avoid_obstacles.py:26-36,122-133) -> abrk_obstacles_params."""
    obs = np.zeros((0, 4)) if obstacles is None or len(obstacles) == 0 else np.asarray(obstacles, dtype=float)
    if obs.ndim != 2 or obs.shape[1] != 4:
        raise ValueError("obstacles must be a list of [x, y, z, radius]")
    if obs.shape[0] > MAX_OBSTACLES:
        raise ValueError(f"at most {MAX_OBSTACLES} obstacles")
    p = ObstaclesParams()
    p.n_obstacles = obs.shape[0]
    p.threshold, p.gain, p.maximum = float(threshold), float(gain), float(maximum)
    for i in range(obs.shape[0]):
        for r in range(4):
            p.obstacles[i][r] = obs[i, r]
    return p


class TwoLinkPlant(C.Structure):
    _fields_ = [("K1", C.c_double), ("K2", C.c_double), ("K3", C.c_double), ("K4", C.c_double), ("dt", C.c_double)]


def make_twolink_plant(L, M_LINKS, dt=0.001):
    """The constants ArmSim.__init__ derives from robot_config.L / _M_LINKS
    (abr_control/arms/twojoint/arm_sim.py:26-41), expression for expression."""
    L = np.asarray(L, dtype=float)
    M = M_LINKS
    Ls = [np.sum(L[ii * 2: ii * 2 + 2]) for ii in range(int(L.shape[0] / 2))]
    p = TwoLinkPlant()
    p.K1 = (1 / 3.0 * M[1][0, 0] + M[2][0, 0]) * Ls[1] ** 2.0 + 1 / 3.0 * M[2][0, 0] * Ls[2] ** 2.0
    p.K2 = M[2][0, 0] * Ls[1] * Ls[2]
    p.K3 = 1 / 3.0 * M[2][0, 0] * Ls[2] ** 2.0
    p.K4 = 1 / 2.0 * M[2][0, 0] * Ls[1] * Ls[2]
    p.dt = dt
    return p


class PathParams(C.Structure):
    """abrk_path_params (include/abrk.h)"""
    _fields_ = [("dt", C.c_double), ("n_samples", C.c_int32), ("n_candidates", C.c_int32), ("axes", C.c_int32),
                ("width", C.c_int32), ("table_len", C.c_int64)]


# the 24 Euler axis sequences as (firstaxis, parity, repetition, frame), the encoding of utils/transformations.py
EULER_AXES = {
    "sxyz": (0, 0, 0, 0), "sxyx": (0, 0, 1, 0), "sxzy": (0, 1, 0, 0), "sxzx": (0, 1, 1, 0), "syzx": (1, 0, 0, 0),
    "syzy": (1, 0, 1, 0), "syxz": (1, 1, 0, 0), "syxy": (1, 1, 1, 0), "szxy": (2, 0, 0, 0), "szxz": (2, 0, 1, 0),
    "szyx": (2, 1, 0, 0), "szyz": (2, 1, 1, 0), "rzyx": (0, 0, 0, 1), "rxyx": (0, 0, 1, 1), "ryzx": (0, 1, 0, 1),
    "rxzx": (0, 1, 1, 1), "rxzy": (1, 0, 0, 1), "ryzy": (1, 0, 1, 1), "rzxy": (1, 1, 0, 1), "ryxy": (1, 1, 1, 1),
    "ryxz": (2, 0, 0, 1), "rzxz": (2, 0, 1, 1), "rxyz": (2, 1, 0, 1), "rzyz": (2, 1, 1, 1),
}


def euler_axes_code(axes):
    """`axes` (one of the 24 strings, or the tuple) as the int the path kernels decode:
    firstaxis | parity << 2 | repetition << 3 | frame << 4"""
    try:
        t = EULER_AXES[axes.lower()]
    except (AttributeError, KeyError):
        t = tuple(int(v) for v in axes) if not isinstance(axes, str) else None
        if t not in EULER_AXES.values():
            raise ValueError(f"axes {axes!r} is none of the 24 Euler axis sequences") from None
    return t[0] | t[1] << 2 | t[2] << 3 | t[3] << 4


class PlantParams(C.Structure):
    """abrk_plant_params (include/abrk.h)"""
    _fields_ = [("dt", C.c_double), ("substeps", C.c_int32), ("gravity", C.c_int32)]


def make_plant_params(dt, substeps=1, gravity=True):
    """One plant step of `dt`, taken as `substeps` Euler steps of dt / substeps with the torques held."""
    p = PlantParams()
    p.dt = float(dt)
    p.substeps = int(substeps)
    p.gravity = int(bool(gravity))
    return p


FX_SATURATION, FX_VISCOUS, FX_COULOMB, FX_LIMITS = 1, 2, 4, 8  # ABRK_FX_* (include/abrk.h)


class PlantEffects(C.Structure):
    """abrk_plant_effects (include/abrk.h)"""
    _fields_ = [("flags", C.c_uint32), ("damping", C.c_double * MAX_JOINTS), ("coulomb", C.c_double * MAX_JOINTS),
                ("coulomb_vs", C.c_double), ("tau_max", C.c_double * MAX_JOINTS), ("q_min", C.c_double * MAX_JOINTS),
                ("q_max", C.c_double * MAX_JOINTS), ("restitution", C.c_double)]


def make_plant_effects(n, damping=None, coulomb=None, coulomb_vs=None, tau_max=None, q_min=None, q_max=None,
                       restitution=0.0):
    """The non-ideal effects of engine.plant_step / forward_dynamics for an arm of `n` joints.  Each per-joint argument
    is a scalar (every joint) or a sequence of n values; None leaves the effect's flag off.  damping: viscous friction
    -b dq; coulomb with coulomb_vs: -c dq / sqrt(dq^2 + vs^2); tau_max: |u| clamped; q_min and q_max (both): hard joint
    limits with the coefficient of restitution `restitution`.  The values are checked by the C entry point."""
    n = int(n)
    if not 1 <= n <= MAX_JOINTS:
        raise ValueError(f"n={n} outside 1..{MAX_JOINTS}")
    p = PlantEffects()

    def fill(field, value, name):
        v = np.asarray(value, dtype=float)
        if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != n):
            raise ValueError(f"{name} must be a scalar or {n} values, got shape {v.shape}")
        for i, x in enumerate(np.broadcast_to(v, (n,))):
            field[i] = x

    if damping is not None:
        fill(p.damping, damping, "damping")
        p.flags |= FX_VISCOUS
    if coulomb is not None:
        if coulomb_vs is None:
            raise ValueError("coulomb friction needs coulomb_vs, the speed below which it fades to zero")
        fill(p.coulomb, coulomb, "coulomb")
        p.coulomb_vs = float(coulomb_vs)
        p.flags |= FX_COULOMB
    elif coulomb_vs is not None:
        p.coulomb_vs = float(coulomb_vs)
    if tau_max is not None:
        fill(p.tau_max, tau_max, "tau_max")
        p.flags |= FX_SATURATION
    if (q_min is None) != (q_max is None):
        raise ValueError("joint limits need both q_min and q_max")
    if q_min is not None:
        fill(p.q_min, q_min, "q_min")
        fill(p.q_max, q_max, "q_max")
        p.flags |= FX_LIMITS
    p.restitution = float(restitution)
    return p


class TraceParams(C.Structure):
    """abrk_trace_params (include/abrk.h)"""
    _fields_ = [("frame", C.c_int32), ("x_off", C.c_double * 3), ("every", C.c_int32), ("capacity", C.c_int32),
                ("columns", C.c_uint32), ("tol", C.c_double)]


# history columns of abrk_loop_trace_batch in their fixed order: name -> (ABRK_TR_* bit, width for n joints)
TRACE_COLUMNS = {"q": (1 << 0, lambda n: n), "dq": (1 << 1, lambda n: n), "u": (1 << 2, lambda n: n),
                 "target": (1 << 3, lambda n: 6), "xyz": (1 << 4, lambda n: 3), "err": (1 << 5, lambda n: 1)}


def trace_columns_mask(columns):
    """column names (any order, no repeats) -> the ABRK_TR_* mask"""
    mask = 0
    for c in columns:
        if c not in TRACE_COLUMNS:
            raise ValueError(f"unknown history column {c!r}: one of {tuple(TRACE_COLUMNS)}")
        if mask & TRACE_COLUMNS[c][0]:
            raise ValueError(f"history column {c!r} named twice")
        mask |= TRACE_COLUMNS[c][0]
    return mask


def trace_layout(mask, n):
    """-> ({name: (first column, width)} of the selected columns in history order, W)"""
    out, o = {}, 0
    for name, (bit, width) in TRACE_COLUMNS.items():
        if mask & bit:
            out[name] = (o, width(n))
            o += width(n)
    return out, o


def make_trace_params(frame, x_off=None, every=1, capacity=0, columns=("xyz", "err"), tol=1e-3):
    """Parameters of engine.loop_trace: `frame` as frame_id() numbers it, `columns` a tuple of names or a mask."""
    p = TraceParams()
    p.frame = int(frame)
    for r in range(3):
        p.x_off[r] = 0.0 if x_off is None else float(x_off[r])
    p.every = int(every)
    p.capacity = int(capacity)
    p.columns = int(columns) if isinstance(columns, (int, np.integer)) else trace_columns_mask(columns)
    p.tol = float(tol)
    return p


CONTACT_MAX_SURFACES = 4  # ABRK_CONTACT_MAX_SURFACES (include/abrk.h)
CONTACT_SURFACE = ("nx", "ny", "nz", "d", "k", "c", "mu", "rho")  # the columns of surface [B,S,8]


class ContactParams(C.Structure):
    """abrk_contact_params (include/abrk.h)"""
    _fields_ = [("frame", C.c_int32), ("off", C.c_double * 3), ("n_surfaces", C.c_int32), ("vs", C.c_double),
                ("accumulate", C.c_int32)]


def make_contact_params(n, frame="EE", offset=(0, 0, 0), n_surfaces=1, vs=1e-3, accumulate=False):
    """Parameters of contact.contact_step for an arm of `n` joints: `frame` a name robot_config.Tx accepts ("EE",
    "link{i}", "joint{i}") or the number frame_id() gives it, `offset` the tool offset in that frame, `n_surfaces` the
    half-spaces per row (1..4), `vs` the smoothing speed of the friction law (m/s), `accumulate`: tau += instead of
    tau =.  The values are checked by the C entry point."""
    p = ContactParams()
    p.frame = int(frame) if isinstance(frame, (int, np.integer)) else frame_id(frame, int(n))
    off = np.asarray(offset, dtype=float)
    if off.shape != (3,):
        raise ValueError(f"offset has shape {off.shape}; expected (3,)")
    for r in range(3):
        p.off[r] = off[r]
    p.n_surfaces = int(n_surfaces)
    p.vs = float(vs)
    p.accumulate = int(bool(accumulate))
    return p


FORCE_CMD = ("nx", "ny", "nz", "f_des")  # the columns of cmd [B,4]
FORCE_GAINS = ("kp", "kv", "kf", "ki", "i_max", "kvf", "f_touch", "v_app", "kv_null")


class ForceParams(C.Structure):
    """abrk_force_params (include/abrk.h)"""
    _fields_ = [("frame", C.c_int32), ("off", C.c_double * 3)] + [(k, C.c_double) for k in FORCE_GAINS] + [
        ("dt", C.c_double), ("use_g", C.c_int32), ("accumulate", C.c_int32), ("force_ld", C.c_int32)]


def make_force_params(n, frame="EE", offset=(0, 0, 0), kp=100.0, kv=20.0, kf=0.5, ki=20.0, i_max=50.0, kvf=20.0,
                      f_touch=0.5, v_app=0.05, kv_null=10.0, dt=0.001, use_g=True, accumulate=False, force_ld=3):
    """Parameters of force_control.force_control_step for an arm of `n` joints: `frame` / `offset` the controlled point
    as in make_contact_params; kp, kv the motion gains; kf, ki, i_max the force PI loop and its anti-windup clamp; kvf
    the damping along the normal while in contact; f_touch (N) the sensed normal force above which a row is in
    contact; v_app (m/s) the approach speed while free; kv_null the null-space damping (0: off); dt (s) the tick;
    use_g: u -= g(q); accumulate: u += instead of u =; force_ld: values per row of the force array (8: a contact
    report).  The values are checked by the C entry point."""
    p = ForceParams()
    p.frame = int(frame) if isinstance(frame, (int, np.integer)) else frame_id(frame, int(n))
    off = np.asarray(offset, dtype=float)
    if off.shape != (3,):
        raise ValueError(f"offset has shape {off.shape}; expected (3,)")
    for r in range(3):
        p.off[r] = off[r]
    p.kp, p.kv, p.kf, p.ki, p.i_max = float(kp), float(kv), float(kf), float(ki), float(i_max)
    p.kvf, p.f_touch, p.v_app, p.kv_null, p.dt = float(kvf), float(f_touch), float(v_app), float(kv_null), float(dt)
    p.use_g = int(bool(use_g))
    p.accumulate = int(bool(accumulate))
    p.force_ld = int(force_ld)
    return p


LINK_CONTACT_MAX_OBSTACLES = 8  # ABRK_LINK_CONTACT_MAX_OBSTACLES (include/abrk.h)
LINK_CONTACT_MAX_SEGMENTS = 7
LINK_OBSTACLE = ("cx", "cy", "cz", "R", "k", "c", "mu")  # the columns of obstacle [B,K,7]


class LinkContactParams(C.Structure):
    """abrk_link_contact_params (include/abrk.h)"""
    _fields_ = [("n_obstacles", C.c_int32), ("link_radius", C.c_double * 7), ("vs", C.c_double),
                ("accumulate", C.c_int32)]


def make_link_contact_params(n, n_obstacles=1, link_radius=0.04, vs=1e-3, accumulate=False):
    """Parameters of link_contact.link_contact_step for an arm of `n` joints: `n_obstacles` the spheres per row (1..8),
    `link_radius` the radius of the segment capsules, a scalar or `n` values (< 0: that segment is off), `vs` the
    smoothing speed of the friction law (m/s), `accumulate`: tau += instead of tau =.  The values are checked by the C
    entry point."""
    p = LinkContactParams()
    p.n_obstacles = int(n_obstacles)
    r = np.asarray(link_radius, dtype=float)
    if r.ndim == 0:
        r = np.full(int(n), float(r))
    if r.shape != (int(n),):
        raise ValueError(f"link_radius has shape {r.shape}; expected a scalar or ({int(n)},)")
    for i in range(LINK_CONTACT_MAX_SEGMENTS):
        p.link_radius[i] = r[i] if i < int(n) else -1.0
    p.vs = float(vs)
    p.accumulate = int(bool(accumulate))
    return p


ADAPT_LIF, ADAPT_LIF_RATE = 0, 1  # ABRK_ADAPT_* (include/abrk.h)
ADAPT_NEURON_TYPES = {"lif": ADAPT_LIF, "lif_rate": ADAPT_LIF_RATE}
ADAPT_MAX_INPUT, ADAPT_MAX_OUTPUT = 64, 16
ADAPT_TAU_PRE = 0.005


class AdaptParams(C.Structure):
    """abrk_adapt_params (include/abrk.h)"""
    _fields_ = [("n_input", C.c_int32), ("n_output", C.c_int32), ("n_neurons_total", C.c_int32),
                ("n_per_ensemble", C.c_int32), ("neuron_type", C.c_int32), ("dt", C.c_double),
                ("tau_input", C.c_double), ("tau_training", C.c_double), ("tau_output", C.c_double),
                ("tau_rc", C.c_double), ("tau_ref", C.c_double), ("pes_learning_rate", C.c_double)]


class AdaptState(C.Structure):
    """abrk_adapt_state (include/abrk.h): the seven per-row state arrays"""
    _fields_ = [(k, C.c_void_p) for k in ("x_f", "e_f", "v", "ref", "a_f", "W", "out_f")]


def make_adapt_params(n_input, n_output, n_neurons=1000, n_ensembles=1, neuron_type="lif", dt=0.001, tau_input=0.012,
                      tau_training=0.012, tau_output=0.2, tau_rc=0.02, tau_ref=0.002, pes_learning_rate=1e-6):
    """Parameters of engine.adapt_step: `n_ensembles` ensembles of `n_neurons` LIF neurons each ("lif": spiking,
    "lif_rate": their rates; or the ABRK_ADAPT_* number) from n_input inputs to n_output outputs.  The defaults are the
    reference's DynamicsAdaptation and Nengo's LIF.  The values are checked by the C entry point."""
    p = AdaptParams()
    p.n_input, p.n_output = int(n_input), int(n_output)
    p.n_per_ensemble = int(n_neurons)
    p.n_neurons_total = int(n_neurons) * int(n_ensembles)
    if isinstance(neuron_type, str):
        if neuron_type not in ADAPT_NEURON_TYPES:
            raise ValueError(f"unknown neuron_type {neuron_type!r}: one of {tuple(ADAPT_NEURON_TYPES)}")
        neuron_type = ADAPT_NEURON_TYPES[neuron_type]
    p.neuron_type = int(neuron_type)
    p.dt = float(dt)
    p.tau_input, p.tau_training, p.tau_output = float(tau_input), float(tau_training), float(tau_output)
    p.tau_rc, p.tau_ref = float(tau_rc), float(tau_ref)
    p.pes_learning_rate = float(pes_learning_rate)
    return p


def lif_gain_bias(intercepts, max_rates, tau_rc=0.02, tau_ref=0.002):
    """Nengo's LIF.gain_bias: the gain and bias with which a neuron starts firing at enc . x = intercept and fires at
    max_rate at enc . x = 1.  With x = 1 / (1 - exp((tau_ref - 1 / max_rate) / tau_rc)): gain = (1 - x) / (intercept - 1),
    bias = 1 - gain * intercept."""
    intercepts, max_rates = np.asarray(intercepts, dtype=float), np.asarray(max_rates, dtype=float)
    if np.any(max_rates >= 1.0 / tau_ref):
        raise ValueError(f"max_rates must be below 1 / tau_ref = {1.0 / tau_ref:g}")
    if np.any(intercepts >= 1.0):
        raise ValueError("intercepts must be below 1")
    x = 1.0 / (1.0 - np.exp((tau_ref - 1.0 / max_rates) / tau_rc))
    gain = (1.0 - x) / (intercepts - 1.0)
    return gain, 1.0 - gain * intercepts


CHANNEL_MAX_WIDTH, CHANNEL_MAX_DELAY = 16, 4096  # ABRK_CHANNEL_* (include/abrk.h)


class ChannelParams(C.Structure):
    """abrk_channel_params (include/abrk.h)"""
    _fields_ = [("width", C.c_int32), ("delay", C.c_int32), ("seed", C.c_uint64), ("row_offset", C.c_int64),
                ("dt", C.c_double), ("tau_diff", C.c_double), ("bias", C.c_double * CHANNEL_MAX_WIDTH),
                ("sigma", C.c_double * CHANNEL_MAX_WIDTH), ("resolution", C.c_double * CHANNEL_MAX_WIDTH)]


class ChannelState(C.Structure):
    """abrk_channel_state (include/abrk.h): the tick counter and the three per-row state arrays"""
    _fields_ = [(k, C.c_void_p) for k in ("counter", "ring", "prev", "d_f")]


def make_channel_params(width, bias=0.0, sigma=0.0, resolution=0.0, delay=0, seed=0, row_offset=0, dt=0.001,
                        tau_diff=0.0):
    """Parameters of sensing.channel_step: `width` columns; bias, sigma (noise standard deviation) and resolution
    (quantisation step) are scalars or one value per column; delay in whole ticks; seed (uint64) and row_offset (the
    global number of row 0) select the noise; dt and tau_diff belong to the differenced output.  The values are checked
    by the C entry point; only what cannot be stored is refused here."""
    width = int(width)
    if not 1 <= width <= CHANNEL_MAX_WIDTH:
        raise ValueError(f"width={width} outside 1..{CHANNEL_MAX_WIDTH}")
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"seed={seed} is not a 64-bit unsigned value")
    p = ChannelParams()
    p.width, p.delay = width, int(delay)
    p.seed, p.row_offset = int(seed), int(row_offset)
    p.dt, p.tau_diff = float(dt), float(tau_diff)
    for name, val in (("bias", bias), ("sigma", sigma), ("resolution", resolution)):
        col = np.asarray(val, dtype=float)
        if col.ndim > 1 or (col.ndim == 1 and col.shape[0] != width):
            raise ValueError(f"{name}: a scalar or {width} values, got shape {col.shape}")
        getattr(p, name)[:width] = np.broadcast_to(col, (width,)).tolist()
    return p


TABLE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "arms", "tables")
BUILTIN_ARMS = ("ur5", "jaco2", "twojoint", "threejoint", "onejoint")


def load_table(name):
    """Arm table (dict) of a built-in arm; see tools/extract_arm_table.py for provenance."""
    with open(os.path.join(TABLE_DIR, f"{name}.json")) as fh:
        return json.load(fh)


def desc_from_table(tab):
    n = int(tab["n_joints"])
    if not 1 <= n <= MAX_JOINTS:
        raise ValueError(f"n_joints={n} outside 1..{MAX_JOINTS}")
    d = ArmDesc()
    d.n_joints = n
    d.n_links_dyn = int(tab["n_links_dyn"])
    d.has_ee = int(tab["has_ee"])
    ident = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]

    def put(dst, m):
        flat = np.asarray(m, dtype=np.float64).reshape(12)
        for i in range(12):
            dst[i] = flat[i]

    put(d.A0, tab["A0"])
    for i in range(MAX_JOINTS):
        put(d.AJ[i], tab["AJ"][i] if i < n else ident)
        put(d.B[i], tab["B"][i] if i < n else ident)
    put(d.E, tab["E"])
    for l in range(MAX_JOINTS + 1):
        row = tab["mdiag"][l] if l < len(tab["mdiag"]) else [0.0] * 6
        for r in range(6):
            d.mdiag[l][r] = float(row[r])
    d.name = tab.get("name", "robot").encode()[:31]
    return d


def _inertia_list(tab, key, count, what):
    """the 6x6 matrices of `tab[key]` as float arrays (exactly `count` of them), checked for symmetry"""
    mats = [np.asarray(m, dtype=np.float64) for m in tab[key]]
    if len(mats) != count or any(m.shape != (6, 6) for m in mats):
        raise ValueError(f"{key}: expected {count} matrices of 6x6 ({what})")
    for i, m in enumerate(mats):
        if not np.all(np.isfinite(m)):
            raise ValueError(f"{key}[{i}] has non-finite entries")
        if not np.array_equal(m, m.T):
            raise ValueError(f"{key}[{i}] is not symmetric: inertia matrices must be (M == M.T, exactly)")
    return mats


def normalize_table(tab):
    """Validate the optional full inertias of an arm table and return the table the kernels run:
    `mlink` (n_joints + 1 matrices, 6x6: the reference's _M_LINKS) and `mjoint` (n_joints matrices: _M_JOINTS).
    An arm is general-inertia only if some `mlink` has an off-diagonal entry or some `mjoint` is non-zero; otherwise the
    plain table (`mdiag` only) is returned - same kernels, same results, same plugin cache key as without the keys.
    Raises ValueError for an asymmetric matrix or a diagonal `mlink` that differs from `mdiag`."""
    if "mlink" not in tab and "mjoint" not in tab:
        return tab
    n = int(tab["n_joints"])
    md = [np.asarray(tab["mdiag"][l] if l < len(tab["mdiag"]) else [0.0] * 6, dtype=np.float64) for l in range(n + 1)]
    ml = _inertia_list(tab, "mlink", n + 1, "one per link, link0 included") if "mlink" in tab else None
    mj = _inertia_list(tab, "mjoint", n, "one per joint") if "mjoint" in tab else None
    off = False
    if ml is not None:
        for l, m in enumerate(ml):
            if np.any(m != np.diag(np.diag(m))):
                off = True
            elif not np.array_equal(np.diag(m), md[l]):
                raise ValueError(f"mlink[{l}] is diagonal but differs from mdiag[{l}]")
    gi = off or (mj is not None and any(np.any(m != 0) for m in mj))
    out = {k: v for k, v in tab.items() if k not in ("mlink", "mjoint")}
    if gi:
        out["mlink"] = [m.tolist() for m in ml] if ml is not None else [np.diag(d).tolist() for d in md]
        out["mjoint"] = [m.tolist() for m in mj] if mj is not None else [[[0.0] * 6] * 6] * n
    return out


def is_general_inertia(tab):
    """True for a table with full link inertias or joint inertias that the plain form cannot express"""
    return "mlink" in normalize_table(tab)


def inertia_from_table(tab):
    """abrk_arm_inertia of a table: its full inertias, or the plain form (diag(mdiag), zero joint inertias)"""
    t = normalize_table(tab)
    n = int(t["n_joints"])
    out = ArmInertia()
    for l in range(n + 1):
        m = np.asarray(t["mlink"][l], dtype=np.float64) if "mlink" in t else np.diag(
            np.asarray(t["mdiag"][l] if l < len(t["mdiag"]) else [0.0] * 6, dtype=np.float64))
        for e in range(36):
            out.mlink[l][e] = m.reshape(36)[e]
    if "mjoint" in t:
        for j in range(n):
            m = np.asarray(t["mjoint"][j], dtype=np.float64).reshape(36)
            for e in range(36):
                out.mjoint[j][e] = m[e]
    return out


def render_tab_struct(t, struct_name, name=None):
    """C++ source of the constexpr arm table `struct <struct_name>` the StaticArm kernels are instantiated on
    (abrk_arms_builtin.h for the built-in arms, the plugin source of a compiled user arm).  Literals are `repr`
    of the doubles, i.e. they read back to exactly the values of the table."""
    def lit(v):
        return repr(float(v))

    def mat(m):
        return "{" + ", ".join(lit(v) for row in m for v in row) + "}"

    ident = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]
    t = normalize_table(t)
    n = int(t["n_joints"])
    md = [list(r) for r in t["mdiag"]] + [[0.0] * 6] * (n + 1 - len(t["mdiag"]))
    out = [
        f"struct {struct_name} {{",
        f"  static constexpr int N = {n};",
        f"  static constexpr int NL = {int(t['n_links_dyn'])};",
        f"  static constexpr bool kHasEE = {'true' if t['has_ee'] else 'false'};",
        f"  static constexpr double A0[12] = {mat(t['A0'])};",
        f"  static constexpr double AJ[{n}][12] = {{" + ",\n      ".join(mat(m) for m in t["AJ"][:n]) + "};",
        f"  static constexpr double B[{n}][12] = {{" + ",\n      ".join(mat(m) for m in t["B"][:n]) + "};",
        f"  static constexpr double E[12] = {mat(t['E'] if t['has_ee'] else ident)};",
        f"  static constexpr double MD[{n + 1}][6] = {{" + ",\n      ".join(
            "{" + ", ".join(lit(v) for v in row) + "}" for row in md[: n + 1]) + "};",
    ]
    if "mlink" in t:  # general inertias (abrk_device.h StaticArm::kGI): full link inertias ML, joint inertias MJ
        out += [
            "  static constexpr bool kGI = true;",
            f"  static constexpr double ML[{n + 1}][36] = {{" + ",\n      ".join(mat(m) for m in t["mlink"]) + "};",
            f"  static constexpr double MJ[{n}][36] = {{" + ",\n      ".join(mat(m) for m in t["mjoint"]) + "};",
        ]
    out += [
        f'  static constexpr const char* kName = "{name if name is not None else t.get("name", "robot")}";',
        "};",
    ]
    return "\n".join(out)


def table_from_desc(d):
    n = d.n_joints
    m = lambda a: np.array(list(a), dtype=np.float64).reshape(3, 4).tolist()
    return {
        "name": d.name.decode(),
        "n_joints": n,
        "n_links_dyn": d.n_links_dyn,
        "has_ee": d.has_ee,
        "A0": m(d.A0),
        "AJ": [m(d.AJ[i]) for i in range(n)],
        "B": [m(d.B[i]) for i in range(n)],
        "E": m(d.E),
        "mdiag": [list(d.mdiag[l]) for l in range(n + 1)],
    }


def frame_id(name, n_joints):
    """'link{i}' -> 2i, 'joint{i}' -> 2i+1, 'EE' -> 2n+1; anything else raises exactly
    like the reference (`Exception("Invalid transformation name: ...")`,
    abr_control/arms/ur5/config.py:337)."""
    try:
        if name == "EE":
            return 2 * n_joints + 1
        if name.startswith("link"):
            i = int(name[4:])
            if 0 <= i <= n_joints:
                return 2 * i
        elif name.startswith("joint"):
            i = int(name[5:])
            if 0 <= i < n_joints:
                return 2 * i + 1
    except (ValueError, AttributeError):
        pass
    raise Exception(f"Invalid transformation name: {name}")


def make_osc_params(
    n_joints,
    kp=1,
    ko=None,
    kv=None,
    ki=0,
    vmax=None,
    ctrlr_dof=None,
    null_controllers=(),
    use_g=True,
    use_C=False,
    orientation_algorithm=0,
    ref_frame="EE",
    xyz_offset=None,
):
    """OSC.__init__ defaults (abr_control/controllers/osc.py:53-118) -> abrk_osc_params."""
    p = OSCParams()
    p.kp = kp
    p.ko = kp if ko is None else ko
    p.kv = float(np.sqrt(p.kp + p.ko)) if kv is None else kv
    p.ki = ki
    p.use_vmax = int(vmax is not None)
    if vmax is not None:
        p.vmax[0], p.vmax[1] = float(vmax[0]), float(vmax[1])
    if ctrlr_dof is None:
        ctrlr_dof = [True, True, True, False, False, False]
    for r in range(6):
        p.ctrlr_dof[r] = int(bool(ctrlr_dof[r]))
    p.use_g = int(bool(use_g))
    p.use_C = int(bool(use_C))
    p.orientation_algorithm = int(orientation_algorithm)
    p.ref_frame = frame_id(ref_frame, n_joints)
    if xyz_offset is not None:
        for r in range(3):
            p.xyz_offset[r] = float(xyz_offset[r])
    null_controllers = list(null_controllers or ())
    if len(null_controllers) > MAX_NULL:
        raise ValueError(f"at most {MAX_NULL} fused null controllers")
    p.n_null = len(null_controllers)
    for i, nc in enumerate(null_controllers):
        p.null_ctrl[i] = nc
    return p


def make_damping(kv):
    c = NullCtrl()
    c.kind = NULL_DAMPING
    c.kv = kv
    return c


def make_resting(rest_angles, kp=1, kv=None):
    """RestingConfig(rest_angles, kp, kv) (resting_config.py:18-23; Joint defaults
    joint.py:26-33: kv = sqrt(kp))."""
    c = NullCtrl()
    c.kind = NULL_RESTING
    c.kp = kp
    c.kv = float(np.sqrt(kp)) if kv is None else kv
    for i, v in enumerate(rest_angles):
        c.rest_mask[i] = int(v is not None)
        c.rest_angles[i] = 0.0 if v is None else float(v)
    return c


def make_joint(kp=1, kv=None):
    c = NullCtrl()
    c.kind = 0
    c.kp = kp
    c.kv = float(np.sqrt(kp)) if kv is None else kv
    return c


def make_sliding_params(n_joints, kd=160.0, lamb=30.0, cartesian=True, ref_frame="EE", offset=None):
    p = SlidingParams()
    p.kd, p.lamb = kd, lamb
    p.cartesian = int(bool(cartesian))
    p.ref_frame = frame_id(ref_frame, n_joints)
    if offset is not None:
        for r in range(3):
            p.offset[r] = float(offset[r])
    return p
