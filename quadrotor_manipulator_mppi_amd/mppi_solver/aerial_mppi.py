"""Aerial-manipulator MPPI: the 6-DoF quadrotor carrying the Kinova arm, sampled as one vehicle.

The reference has no controller for the vehicle it is named after (``README.md:33`` TODO): its drone
solver moves a point mass and its arm solver holds the base still.  This class samples the
quadrotor's thrust and body torques together with the seven joint accelerations (``A = 11``) and costs
the end effector under the attitude each sampled rollout actually has:

    EE(k,t) = [Rz(yaw) Ry(pitch) Rx(roll) | p](k,t) M_fixed chain(q(k,t))

with the base stepped by the quadrotor model (``quadrotor_mppi``: the commented loop of
``drone_mppi.py:57-83``) and the joints by the arm's double integrator (``mppi.py``).  The coupling is
kinematic only: ``mass`` and ``inertia`` are the loaded vehicle's, and arm motion does not react on the base.

Surface: ``set_state(x, v)`` as ``quadrotor_mppi`` (x = (xyz, rpy), v = (world velocity, body rates)),
``update_joint(q, qd)`` (seven joint angles and rates), ``compute_control_input() -> (x_des, v_des, qdes,
vdes)`` -- the base's first step under the new u[0] as ``quadrotor_mppi`` returns it (torch (6,) tensors on
``self.device``) and the arm's ``qdes``, ``vdes`` as ``mppi.py:157-158`` (numpy (7,)) -- and the base class's
``get_plan`` / ``get_elites`` / ``get_trajectory`` (rows: xyz, rpy, q, EE 4x4).  The pose target is
``target_pose`` as the arm class has it.  The warm start begins at hover thrust m*g.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..engine import make_config
from ..robot.urdf_chain import load_chain, parse_urdf_chain
from ..utils.pose import Pose
from ._base import OutputRing, SolverBase


class MPPI(SolverBase):
    def __init__(self, n_samples: int = 100, n_horizon: int = 32, device: Optional[int] = None,
                 noise: str = "philox", seed: int = 0x5EED, mass: float = 14.7, inertia=(1.57, 3.93, 2.59),
                 kd: float = 0.0, gravity: float = 9.81, urdf_path: Optional[str] = None, root_link: str = "base",
                 end_link: str = "j2s7s300_link_7", verbose: bool = False, prewarm_us: int = 0,
                 track_target: bool = False, scene=None, field=None, self_collision=None, limits=None):
        """``limits``: an ``engine.Limits`` (or True: thrust within [0, 2 m g], torques unbounded) bounds thrust and
        body torques in the rollouts, the plan and the returned u; ``set_limits`` replaces the values."""
        for what, given in (("self-collision pairs", self_collision is not None), ("distance fields", field is not None),
                            ("obstacle scenes", scene is not None), ("target trajectories", bool(track_target))):
            if given:
                raise NotImplementedError(f"{what} are not available for the aerial manipulator model (its rollout "
                                          "kernel runs the pose cost alone); use the arm class")
        super().__init__(11, n_horizon, device, noise, seed, verbose, prewarm_us)
        self._limits = limits
        self.n_manipulator_dof = 7
        self.n_samples = n_samples
        self.n_horizon = n_horizon
        self._lambda = 0.1
        self.sigma = torch.diag(torch.tensor([30.0, 1.0, 1.0, 1.0] + [0.1] * 7))
        self.params = dict(quad_mass=mass, quad_inertia=tuple(inertia), quad_kd=kd, quad_gravity=gravity)
        self.chain = parse_urdf_chain(urdf_path, root_link, end_link) if urdf_path else load_chain()
        self.x_prev = torch.zeros(6)
        self.v_prev = torch.zeros(6)
        self._q = np.zeros(7, np.float32)
        self._qdot = np.zeros(7, np.float32)
        self.qdes = None
        self.vdes = None
        self.target_pose = Pose()   # mppi.py:70-72
        self.target_pose.pose = torch.tensor([0.1029, 0.4055, 1.6498])
        self.target_pose.orientation = torch.tensor([-0.5, -0.5, 0.5, -0.5])
        self._u_prev_host[:, 0] = np.float32(mass * gravity)   # hover thrust
        self._row = np.zeros(26, np.float64)   # xyz rpy q | v omega qd
        self._out_ring = OutputRing(self.device, 12)

    def _config(self, key):
        return make_config("aerial", n_samples=key[1], n_horizon=key[2], dt=self.dt, lam=self._lambda,
                           sigma=self.sigma.numpy(), chain=self.chain, seed=self._seed,
                           noise="injected" if key[0] else self._noise, device=self._dev_index, quad=self.params)

    def set_state(self, x, v):
        """x = (xyz, rpy), v = (world velocity, body rates), flat or nested; float32 like drone_mppi.py:179-183."""
        xn = torch.tensor(np.asarray(x, np.float64).reshape(6), dtype=torch.float32)
        vn = torch.tensor(np.asarray(v, np.float64).reshape(6), dtype=torch.float32)
        with self._lock:
            self.x_prev, self.v_prev = xn, vn

    def update_joint(self, q, qd):
        """The arm's seven joint angles and rates (stored as float32)."""
        qn = np.asarray(q, np.float64).reshape(7).astype(np.float32)
        vn = np.asarray(qd, np.float64).reshape(7).astype(np.float32)
        with self._lock:
            self._q, self._qdot = qn, vn

    def compute_control_input(self, noise: Optional[np.ndarray] = None):
        row = self._row
        with self._lock:
            row[:6] = self.x_prev.numpy()
            row[6:13] = self._q
            row[13:19] = self.v_prev.numpy()
            row[19:26] = self._qdot
        eng = self._ensure_engine((noise is not None or self._noise == "injected", self.n_samples, self.n_horizon))
        self._sync_target(eng, self.target_pose.pose.numpy(), self.target_pose.orientation.numpy())
        self._sync_limits(eng)
        out, u0, stats = eng.step(row, noise)
        st = self._after_step(u0, stats)
        if self.verbose:
            print("Rho :", torch.tensor(st.rho))
        t = self._out_ring.to_device(out[0, :12])
        self.qdes = out[0, 12:19].astype(np.float32)
        self.vdes = out[0, 19:26].astype(np.float32)
        return t[:6], t[6:], self.qdes.copy(), self.vdes.copy()

    def compute_weights(self, S: torch.Tensor) -> torch.Tensor:
        return super().compute_weights(S, self._lambda)
