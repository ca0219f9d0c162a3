"""6-DoF rigid-body quadrotor MPPI, shaped like the drone solver.

The reference ships this controller only as the commented-out ``predict_trajectory``
of ``src/mav_mppi/scripts/mppi_solver/drone_mppi.py:57-83`` (thrust along body z plus
body torques, Euler-angle attitude; J and R from ``drone.py:114-154``; m and I from
``aerial_manipulation/urdf/drone.urdf:15-16``).  This class gives it the drone
solver's surface: ``MPPI()``, ``set_state(x, v)`` with x = (xyz, rpy) and
v = (world velocity, body rates), and ``compute_control_input() -> (x_des, v_des)``
as torch (6,) tensors on ``self.device``: the model's first step under the new u[0].
The action is (thrust [N], tau_x, tau_y, tau_z [N m]); the warm start begins at
hover thrust m*g.  Parity is unpinned (no reference output exists): the GPU path is
checked against the torch restatement ``oracle.mppi_oracle.quad_step``.
The class body is ``_base.VehicleSolver``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._base import VehicleSolver


class MPPI(VehicleSolver):
    def __init__(self, n_samples: int = 1000, n_timestep: int = 32, device: Optional[int] = None,
                 noise: str = "philox", seed: int = 0x5EED, mass: float = 14.7,
                 inertia=(1.57, 3.93, 2.59), kd: float = 0.0, gravity: float = 9.81, verbose: bool = False, prewarm_us: int = 0,
                 track_target: bool = False, scene=None, field=None, self_collision=None, limits=None):
        """``limits``: an ``engine.Limits`` (or True: thrust within [0, 2 m g], torques unbounded) bounds thrust and
        body torques in the rollouts, the plan and the returned u; ``set_limits`` replaces the values."""
        if self_collision is not None:
            raise NotImplementedError("self-collision pairs are not available for the 6-DoF quadrotor model "
                                      "(no scene form of its rollout kernel); use the arm class")
        if field is not None:
            raise NotImplementedError("distance fields are not available for the 6-DoF quadrotor model "
                                      "(no scene form of its rollout kernel); use the drone or arm classes")
        if scene is not None:
            raise NotImplementedError("obstacle scenes are not available for the 6-DoF quadrotor model "
                                      "(no scene form of its rollout kernel); use the drone or arm classes")
        super().__init__(6, torch.diag(torch.tensor([30.0, 1.0, 1.0, 1.0])), n_samples, n_timestep,
                         device, noise, seed, verbose, prewarm_us, track_target=track_target, limits=limits)
        self.params = dict(quad_mass=mass, quad_inertia=tuple(inertia), quad_kd=kd, quad_gravity=gravity)
        self._u_prev_host[:, 0] = np.float32(mass * gravity)   # hover thrust

    def set_state(self, x, v):
        """x = (xyz, rpy), v = (world velocity, body rates), flat or nested; float32 like drone_mppi.py:179-183."""
        super().set_state(np.asarray(x, np.float64).reshape(6), np.asarray(v, np.float64).reshape(6))

    def _config(self, key):
        return self._vehicle_config("quadrotor", key, quad=self.params)
