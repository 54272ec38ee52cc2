"""Shapes of a path from start to target (the reference's controllers/path_planners/position_profiles.py).

A position profile maps t in [0, 1] to a 3-vector, from [0, 0, 0] at t = 0 to [1, 1, 1] at t = 1; `PathPlanner` rotates,
stretches and shifts that curve onto the actual start and target.  The profiles are plain host-side Python: the planner
samples `step` once per `generate_path` call (n_sample_points values, shared by every row of a batch) and hands the
table to the device, so a user's own subclass works unchanged."""
import numpy as np


class PosProf:
    """Base class: stores n_sample_points and checks the two end conditions of `step`."""

    def __init__(self, tol=1e-6, n_sample_points=1000, **kwargs):
        self.n_sample_points = n_sample_points
        at0, at1 = self.step(0), self.step(1)
        assert sum(abs(at0)) <= tol, f"Position profile must equal [0, 0, 0] at t=0; step(0) returns {at0}"
        for value in at1:
            assert abs(value - 1) <= tol, f"Position profile must equal [1, 1, 1] at t=1; step(1) returns {at1}"

    def step(self, t):
        """t in [0, 1] -> 3 floats; [0, 0, 0] at 0 and [1, 1, 1] at 1 (within tol)"""
        raise NotImplementedError


class Linear(PosProf):
    """A straight line."""

    def __init__(self, n_sample_points=10, **kwargs):
        super().__init__(n_sample_points=n_sample_points, **kwargs)

    def step(self, t):
        return np.array([t, t, t])


class SinCurve(PosProf):
    """The axes named in `axes` ('x', 'y', 'z') follow a sine from 0 to (4 (cycles - 1) + 1) pi / 2, the others a
    straight line.  `cycles` counts per axis: 1 ends at pi / 2, 2 at 5 pi / 2, ..."""

    def __init__(self, axes=None, cycles=None, n_sample_points=1000, **kwargs):
        self.axes = ["x"] if axes is None else axes
        self.cycles = [1, 1, 1] if cycles is None else cycles
        # cycles become quarter periods in place, as in the reference: a list passed in is changed too
        for index in range(len(self.cycles)):
            self.cycles[index] = (self.cycles[index] - 1) * 4 + 1
        super().__init__(n_sample_points=n_sample_points, **kwargs)

    def step(self, t):
        out = [np.sin(self.cycles[index] * t * np.pi / 2) if name in self.axes else t
               for index, name in enumerate("xyz")]
        return np.array(out)


class FromPoints(PosProf):
    """Linear interpolation through given points: x [N] times in [0, 1], y [3,N] (or [N,3]) positions from [0, 0, 0] to
    [1, 1, 1]."""

    def __init__(self, x, y, n_sample_points=1000, **kwargs):
        import scipy.interpolate

        if y.shape[0] != 3:
            y = y.T
        self.X, self.Y, self.Z = (scipy.interpolate.interp1d(x, y[index]) for index in range(3))
        super().__init__(n_sample_points=n_sample_points, **kwargs)

    def step(self, t):
        if t == 0:
            return np.zeros(3)
        if t == 1:
            return np.ones(3)
        return np.array([self.X(t), self.Y(t), self.Z(t)])


class Ellipse(PosProf):
    """Half an ellipse in the Cartesian plane `plane` ('xy', 'xz', 'yz'): horz_stretch is its half axis perpendicular
    to start -> target (negative: the other side); the third coordinate is a straight line."""

    def __init__(self, horz_stretch, plane="xy", n_sample_points=1000, **kwargs):
        self.indices = {"x": 0, "y": 1, "z": 2}
        self.plane = plane
        for name, index in self.indices.items():
            if name not in self.plane:
                self.linear_index = index
        self.b = horz_stretch
        # the curve is drawn along x, turned by 45 degrees onto the diagonal and stretched to reach [1, 1]
        G = -np.pi / 4
        self.R = np.array([[np.cos(G), -np.sin(G)], [np.sin(G), np.cos(G)]])
        self.mag = 2 * np.sin(-G)
        super().__init__(n_sample_points=n_sample_points, **kwargs)

    def step(self, t):
        # ellipse centred at [0.5, 0] with half axes 0.5 and b, solved for y
        y = self.b * np.sqrt(1 - (t - 0.5) ** 2 / 0.5 ** 2)
        xy = np.dot(np.array([t, y]), self.R) * self.mag
        out = np.zeros(3)
        out[self.indices[self.plane[0]]] = xy[0]
        out[self.indices[self.plane[1]]] = xy[1]
        out[self.linear_index] = t
        return out
