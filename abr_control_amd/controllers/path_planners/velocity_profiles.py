"""Velocity ramps from a start to a target velocity (the reference's controllers/path_planners/velocity_profiles.py).

`generate` returns the 1-D array of speeds, one per time step dt.  Host-side Python: `PathPlanner` calls it once per
candidate maximum velocity and per `generate_path` call, whatever the batch size, and uploads the results."""
import numpy as np


class VelProf:
    """Base class: keeps the time step, which the planner reads."""

    def __init__(self, dt):
        self.dt = dt

    def generate(self, start_velocity, target_velocity):
        """-> 1-D array of velocities from start_velocity to target_velocity"""
        raise NotImplementedError


class Gaussian(VelProf):
    """The rising half of a Gaussian, n_sigma standard deviations wide, shifted to start at start_velocity and scaled
    to end at target_velocity; its length is the time a constant `acceleration` would take."""

    def __init__(self, dt, acceleration, n_sigma=3):
        self.acceleration = acceleration
        self.n_sigma = n_sigma
        super().__init__(dt=dt)

    def generate(self, start_velocity, target_velocity):
        ramp_up_time = (target_velocity - start_velocity) / self.acceleration
        # a Gaussian whose peak is the velocity difference has this sigma
        s = 1 / ((target_velocity - start_velocity) * np.sqrt(np.pi * 2))
        u = self.n_sigma * s
        x = np.linspace(0, u, int(ramp_up_time / self.dt))
        vel_profile = 1 * (1 / (s * np.sqrt(2 * np.pi)) * np.exp(-0.5 * ((x - u) / s) ** 2))
        vel_profile -= vel_profile[0]
        vel_profile *= (target_velocity - start_velocity) / vel_profile[-1]
        vel_profile += start_velocity
        return vel_profile


class Linear(VelProf):
    """A straight ramp of slope `acceleration`."""

    def __init__(self, dt, acceleration):
        self.acceleration = acceleration
        super().__init__(dt=dt)

    def generate(self, start_velocity, target_velocity):
        vdiff = target_velocity - start_velocity
        t = vdiff / self.acceleration
        steps = t / self.dt
        return np.linspace(start_velocity, target_velocity, int(steps))
