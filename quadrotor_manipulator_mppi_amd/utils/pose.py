"""Minimal goal-pose container with the attribute surface of the reference's
``utils/pose.py:4-112`` that the solver API exposes (``target_pose.pose`` xyz,
``target_pose.orientation`` quaternion **xyzw**, ``clone``)."""
import numpy as np
import torch


def _quat_R(x, y, z, w):
    """The rotation matrix of a quaternion xyzw (normalised here): the nodes' base rotation,
    ``pin.XYZQUATToSE3`` at ``kinova.py:113-114`` and ``drone.py:107-109``."""
    n = np.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


class Pose:
    def __init__(self):
        self.pose = torch.zeros(3)
        self.orientation = torch.tensor([0.0, 0.0, 0.0, 1.0])

    @property
    def np_pose(self):
        return self.pose.numpy()

    @property
    def np_orientation(self):
        return self.orientation.numpy()

    def clone(self):
        p = Pose()
        p.pose = self.pose.clone()
        p.orientation = self.orientation.clone()
        return p
