"""Drop-in replacement for the reference's drone solver ``mppi_solver/drone_mppi.py``.

Same surface as ``MPPI`` at ``src/mav_mppi/scripts/mppi_solver/drone_mppi.py:7-183``:
``MPPI()``, ``set_state(x(3,), v(3,))`` (:179-183),
``compute_control_input() -> (x: torch(3,), v: torch(3,))`` on ``self.device``
(:140-176; the caller does ``xdes.to('cpu').tolist()``, drone.py:240),
``compute_weights(S)`` (:111-130) and the attributes ``n_samples, n_timestep,
dt, n_action, sigma, param_lambda, param_gamma, u_prev, u, x_prev, v_prev``.

The step runs in libmppi_hip.so.  The reference prints ``Rho`` on every step
(:123); set ``verbose=True`` to get the same line (off by default: it is I/O in
the control loop).  The class body is ``_base.VehicleSolver``.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._base import VehicleSolver


class MPPI(VehicleSolver):
    def __init__(self, n_samples: int = 1000, n_timestep: int = 32, device: Optional[int] = None,
                 noise: str = "philox", seed: int = 0x5EED, verbose: bool = False, prewarm_us: int = 0,
                 track_target: bool = False, scene=None, field=None, self_collision=None):
        """``track_target``: a target that may move along the horizon (``set_target_trajectory`` with
        (H, 3) positions, ``clear_target_trajectory``); off, the class is as before.  ``scene``: an
        ``engine.Scene`` (True: the placeholder 0.30 m sphere) for obstacle avoidance
        (``set_obstacles``, ``clear_obstacles``).  ``field``: an ``engine.DistanceField``, a voxel
        distance field as one more obstacle (``set_distance_field``, ``clear_distance_field``)."""
        if self_collision is not None:
            raise NotImplementedError("self-collision pairs are not available for the drone model (no chain: every pair "
                                      "of its spheres is rigid); use the arm class")
        super().__init__(3, torch.eye(3) * 30.0, n_samples, n_timestep, device, noise, seed, verbose, prewarm_us,
                         track_target=track_target, scene=scene, field=field)
        self.param_gamma = self.param_lambda * (1.0 - 0.9)

    def _config(self, key):
        return self._vehicle_config("drone", key)

    def apply_constraint(self, u: torch.Tensor) -> torch.Tensor:
        """drone_mppi.py:131-137 (unused by the reference's step)."""
        lim = torch.tensor([10.0, 10.0, 10.0], device=u.device)
        return torch.clamp(u, min=-lim, max=lim)
