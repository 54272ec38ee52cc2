"""Velocity-limited path planner with the reference's interface (abr_control/controllers/path_planners/
path_planner.py:13-475), for one movement or a batch of B independent movements planned on the device.

What runs where (DESIGN.md "Path planner"):
  host, once per generate_path call whatever B is - everything that depends on the profile OBJECTS, through their own
    Python: pos_profile.step sampled at linspace(0, 1, n_sample_points); vel_profile.generate for every candidate
    max_v = max_velocity - 0.1 k (formed by repeated subtraction like the reference's search loop, :242-302), the
    np.sum distances and np.cumsum prefixes of the two ramps.  A user's own PosProf / VelProf subclass therefore works,
    and no libm sin / exp of a profile is re-evaluated by the device.
  device, per row - the warp of the curve onto start -> target, its chord lengths, the choice of the candidate, the
    step count (plan pass); interpolation along the curve, SLERP and Euler angles (fill pass); np.gradient velocities
    and the padding (gradient pass): engine.path_plan / engine.path_fill, csrc/abrk_path.{h,hip}.
The only synchronisation is the read-back of n_timesteps between the two passes, which sizes the output."""
import warnings

import numpy as np

from ... import _abi, engine
from ..._lib import DeviceArray
from .orientation import Orientation


def profile_tables(pos_profile, vel_profile, max_velocity, start_velocity=0, target_velocity=0):
    """The packed table of one generate_path call (layout: include/abrk.h, abrk_path_plan_batch) ->
    (table float64 [len], offsets int64 [2 + 4 K], candidates) with candidates = [(max_v, starting_vel_profile,
    ending_vel_profile, starting_dist, ending_dist), ...] as the reference's search loop would see them in turn.
    The list ends before the first candidate whose ramps cannot be generated (max_v <= 0, or a profile that fails on
    it): a row that would need it has no path."""
    dt = vel_profile.dt
    S = int(pos_profile.n_sample_points)
    samples = np.array([np.asarray(pos_profile.step(t), dtype=np.float64) for t in np.linspace(0, 1, S)])
    samples = samples.reshape(S, 3)
    # the two special cases of path_planner.py:153-163: a ramp that is already at max_velocity is one step long, covers
    # no distance and is kept for every candidate
    starting_dist, starting = (0, [start_velocity * dt]) if start_velocity == max_velocity else (None, None)
    ending_dist, ending = (0, [target_velocity * dt]) if target_velocity == max_velocity else (None, None)
    candidates = []
    max_v = max_velocity
    with np.errstate(all="ignore"):
        while max_v > 0:
            try:
                if starting_dist != 0:
                    starting = vel_profile.generate(start_velocity=start_velocity, target_velocity=max_v)
                    starting_dist = np.sum(starting * dt)
                if ending_dist != 0:
                    if start_velocity == target_velocity:  # mirror instead of generating again (:260-261)
                        ending = starting[::-1]
                    else:
                        ending = vel_profile.generate(start_velocity=target_velocity, target_velocity=max_v)[::-1]
                    ending_dist = np.sum(ending * dt)
            except (IndexError, ZeroDivisionError, ValueError):
                break
            s_arr, e_arr = np.asarray(starting, dtype=np.float64), np.asarray(ending, dtype=np.float64)
            if not (np.all(np.isfinite(s_arr)) and np.all(np.isfinite(e_arr)) and np.isfinite(starting_dist)
                    and np.isfinite(ending_dist)):
                break
            candidates.append((float(max_v), s_arr, e_arr, float(starting_dist), float(ending_dist)))
            max_v -= 0.1
    K = len(candidates)
    parts, offsets, at = [], [], 0

    def put(values):
        nonlocal at
        values = np.ascontiguousarray(values, dtype=np.float64).ravel()
        parts.append(values)
        at += values.size
        return at - values.size

    offsets.append(put(samples))
    offsets.append(put(np.array([[c[0], c[3], c[4]] for c in candidates]).reshape(K, 3)))
    for _, s_arr, e_arr, _, _ in candidates:
        offsets += [put(np.cumsum(s_arr * dt)), s_arr.size, put(np.cumsum(e_arr * dt)), e_arr.size]
    return np.concatenate(parts), np.array(offsets, dtype=np.int64), candidates


class PathPlanner:
    """pos_profile: a position_profiles object (`step(t)`, `n_sample_points`); vel_profile: a velocity_profiles object
    (`generate(start_velocity, target_velocity)`, `dt`); axes: Euler order of the orientations (any of the 24
    sequences).  device / stream: where the batch is planned."""

    def __init__(self, pos_profile, vel_profile, axes="rxyz", verbose=False, device=0, stream=None):
        self.n_sample_points = pos_profile.n_sample_points
        self.dt = vel_profile.dt
        self.pos_profile = pos_profile
        self.vel_profile = vel_profile
        self.axes = axes
        self._axes_code = _abi.euler_axes_code(axes)
        self.OrientationPlanner = Orientation(axes=self.axes)
        self.n = 0
        self.n_timesteps = None
        self.target_counter = 0
        self.verbose = verbose
        self.log = []
        self.device, self.stream = device, stream
        self.starting_vel_profile = None
        self.ending_vel_profile = None
        self.start_velocity = 0
        self.target_velocity = 0
        self._host = np.zeros((12, 1))
        self._dev = None
        self._single = True

    # ---- the generated path: fetched from the device when first asked for
    @property
    def path(self):
        if self._host is None:
            full = self._dev[0].numpy(self.stream)
            self._host = full[0, :int(self.n_timesteps)] if self._single else full
        return self._host

    @property
    def position_path(self):
        return self.path[..., 0:3]

    @property
    def velocity_path(self):
        return self.path[..., 3:6]

    @property
    def orientation_path(self):
        if self.path.shape[-1] != 12:
            raise AttributeError("no orientation path was planned (generate_path without start_orientation)")
        return self.path[..., 6:9]

    @property
    def ang_velocity_path(self):
        if self.path.shape[-1] != 12:
            raise AttributeError("no orientation path was planned (generate_path without start_orientation)")
        return self.path[..., 9:12]

    def device_path(self):
        """-> (path, n_timesteps): the DeviceArrays of the last generate_path - float64 [B, Tmax, 6 | 12] and int32 [B]
        - as engine.path_next takes them; no host round trip"""
        if self._dev is None:
            raise RuntimeError("generate_path has not been called")
        return self._dev

    def align_vectors(self, a, b):
        """the rotation matrix that turns vector a onto vector b (host arithmetic; the kernels carry their own)"""
        b = b / np.linalg.norm(b)
        a = a / np.linalg.norm(a)
        v1, v2, v3 = np.cross(a, b)
        h = 1 / (1 + np.dot(a, b))
        Vmat = np.array([[0, -v3, v2], [v3, 0, -v1], [-v2, v1, 0]])
        return np.eye(3, dtype=np.float64) + Vmat + (Vmat.dot(Vmat) * h)

    def generate_path(self, start_position, target_position, max_velocity, start_orientation=None,
                      target_orientation=None, start_velocity=0, target_velocity=0, plot=False, to_host=True):
        """One movement - start_position, target_position (3,), orientations (3,) Euler angles in `axes` or None ->
        path (T, 6 | 12) as the reference returns it - or a batch: positions (B,3), orientations (B,3) or None ->
        path (B, Tmax, 6 | 12) with n_timesteps an int array (B,); row b is valid in [:n_timesteps[b]] and holds its own
        last point after that.  max_velocity, start_velocity, target_velocity: scalars, shared by the batch.
        Columns: position, velocity (, Euler angles, their time derivative).
        to_host=False leaves the result on the device (returns the DeviceArray; see device_path()); the host attributes
        fetch it when first read.  Raises ValueError when a row has no path (start == target; no reachable max_v)."""
        if plot:
            raise NotImplementedError("plotting is not part of abr_control_amd (headless); plot the returned path yourself")
        assert start_velocity <= max_velocity, f"start velocity({start_velocity}m/s) > max velocity({max_velocity}m/s)"
        assert target_velocity <= max_velocity, f"target velocity({target_velocity}m/s) > max velocity({max_velocity}m/s)"
        self.max_velocity = max_velocity
        self.start_velocity = start_velocity
        self.target_velocity = target_velocity

        single = np.ndim(start_position) == 1
        start = np.ascontiguousarray(np.atleast_2d(np.asarray(start_position, dtype=np.float64)))
        B = start.shape[0]
        target = np.ascontiguousarray(np.broadcast_to(np.atleast_2d(np.asarray(target_position, dtype=np.float64)), (B, 3)))
        if start.shape != (B, 3) or B == 0:
            raise ValueError(f"start_position: expected (3,) or (B,3) with B >= 1, got {np.shape(start_position)}")
        arrays = (list, np.ndarray, np.generic, tuple)
        width = 6
        ori = [None, None]
        if isinstance(start_orientation, arrays):
            if not isinstance(target_orientation, arrays):
                raise NotImplementedError("A target orientation is required to generate path")
            width = 12
            ori = [np.ascontiguousarray(np.broadcast_to(np.atleast_2d(np.asarray(o, dtype=np.float64)), (B, 3)))
                   for o in (start_orientation, target_orientation)]

        table, offsets, candidates = profile_tables(self.pos_profile, self.vel_profile, max_velocity, start_velocity,
                                                    target_velocity)
        if not candidates:
            raise ValueError("no velocity profile can be generated for this max_velocity")
        self._candidates = candidates
        P = _abi.PathParams(float(self.dt), int(self.n_sample_points), len(candidates), self._axes_code, width,
                            int(table.size))
        dev, st = self.device, self.stream
        up = lambda h: None if h is None else DeviceArray.from_numpy(h, dev, getattr(st, "ptr", st))
        d_table, d_start, d_target, d_so, d_to = up(table), up(start), up(target), up(ori[0]), up(ori[1])
        nt_d, rowplan_d, ds_d = engine.path_plan(P, d_table, offsets, d_start, d_target, device=dev, stream=st)
        nt = nt_d.numpy(st)  # the one synchronisation: the step counts size the output
        t_max = int(nt.max())
        path_d = engine.path_fill(P, d_table, offsets, t_max, d_start, d_target, nt_d, rowplan_d, ds_d, d_so, d_to,
                                  device=dev, stream=st)
        self._dev = (path_d, nt_d)
        self._single = single
        self._host = None
        self._rowplan = rowplan_d

        self.n_timesteps = int(nt[0]) if single else nt.astype(np.int64)
        self.n = 0 if single else np.zeros(B, dtype=np.int64)
        self.time_to_converge = self.n_timesteps * self.dt
        self.target_counter += 1
        if single:
            k = int(rowplan_d.numpy(st)[0, 0])
            self.starting_vel_profile, self.ending_vel_profile = candidates[k][1], candidates[k][2]
        if self.verbose:
            print(f"PathPlanner: {B} movement(s), max_velocity={max_velocity}, start_velocity={start_velocity}, "
                  f"target_velocity={target_velocity}, dt={self.dt}, steps {int(nt.min())}..{t_max}")
        if not to_host:
            return path_d
        path = self.path
        last = path[-1, :3] if single else path[np.arange(B), nt - 1, :3]
        err = np.max(np.linalg.norm(np.atleast_2d(last - (target[0] if single else target)), axis=-1))
        if err >= 0.01:
            warnings.warn(
                f"the end of the generated path is {err}m from the desired target position. For a lower error try a "
                "path shape with lower frequency terms, more sample points, a smaller timestep, lower maximum velocity "
                "and acceleration, or lower start and end velocities")
        return path

    def next(self):
        """the next target of the path: (6 | 12,) - or (B, 6 | 12), every row clamped at its own last point"""
        if self._single:
            point = self.path[self.n]
            self.n = min(self.n + 1, self.n_timesteps - 1) if self.n_timesteps is not None else self.n + 1
            return point
        point = self.path[np.arange(len(self.n)), self.n]
        self.n = np.minimum(self.n + 1, self.n_timesteps - 1)
        return point

    def next_at_n(self, n):
        """the nth point of the path (the last one beyond its end); no counter moves"""
        if self._single:
            return self.path[min(n, self.n_timesteps - 1)]
        return self.path[np.arange(len(self.n_timesteps)), np.minimum(n, self.n_timesteps - 1)]

    def convert_to_time(self, path, time_length):
        raise NotImplementedError("convert_to_time is not part of abr_control_amd; interpolate the returned path on the host")

    def _plot(self, start_position, target_position):
        raise NotImplementedError("plotting is not part of abr_control_amd (headless)")
