"""The project's default body spheres and obstacle-term weights (``mppi_scene_default`` in
csrc/mppi_layout.cpp holds the same numbers; tests/test_capi_obstacles_cpu.py compares the two).

Project data, not the reference's: placeholders for the user's collision model.  One sphere at the
frame origin of every actuated chain joint, one on the base frame (-1) of a flying vehicle.
"""
JOINT_SPHERE_RADIUS = 0.05     # m, every actuated joint's frame origin (ARM, WHOLEBODY)
VEHICLE_SPHERE_RADIUS = 0.30   # m, frame -1 (WHOLEBODY, DRONE)
W_OBS, MARGIN, PENALTY = 100.0, 0.05, 1e4
# the self-collision term's own weights (``mppi_self_collision_default``): self margins are tighter
W_SELF, MARGIN_SELF, PENALTY_SELF = 100.0, 0.02, 1e4


def default_body(model: str, chain) -> tuple:
    """((frame, offset, radius), ...) for a model name and its chain (dicts with a "type")."""
    body = [(-1, (0.0, 0.0, 0.0), VEHICLE_SPHERE_RADIUS)] if model in ("wholebody", "drone") else []
    if model in ("arm", "wholebody"):
        body += [(f, (0.0, 0.0, 0.0), JOINT_SPHERE_RADIUS) for f, j in enumerate(chain) if j["type"] != "fixed"]
    return tuple(body)
