"""What a depth frame costs: the map carved and marked on the device from the image (Engine.integrate_depth)
against the route without it -- ray casting on the host, then set_occupancy of the resulting map -- for the
same frame, in the same process (tools/, not shipped).

    python tools/ab_depth.py [reps]          the table
    python tools/ab_depth.py --passes [n]    n integrate_depth calls per case and nothing else: the run to put
                                             under a kernel trace for the per-kernel times

Per grid (128^3 and 64^3 at voxel 0.05; a 640 x 480 frame, fx = fy = 554.25 as the VI-sensor's depth camera,
taken from the centre of a box room that fits the grid, with a pillar in front of the far wall and a few
drop-outs) and per stride (1, 2), wall time around work that ends in a synchronise,
after 5 warm-up calls of each, alternating the two device routes call by call:
  depth       integrate_depth(frame) + synchronize: the image's copy (1.2 MB), carve, mark, the transform's
              four launches, the header
  occupancy   set_occupancy(map) + synchronize on the resulting map: the device side of the other route with
              its host ray casting left out -- a lower bound of what the feature replaces
  host cast   the ray casting the other route needs first: the library's own host twin
              (mppi_depth_integrate_host) for the same frame, 3 runs, for information
Medians and interquartile ranges in microseconds (host cast: milliseconds).  The device map is compared with
the host twin's before anything is timed.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from quadrotor_manipulator_mppi_amd.engine import DepthView, DistanceField, Engine, Scene, depth_integrate_host, make_config
from tools.ab_native import STATE
from tools.ab_obstacles import BODY
from tools.ab_occupancy import stats

GRIDS = [((128, 128, 128), 0.05), ((64, 64, 64), 0.05)]
STRIDES = [1, 2]
MAX_DIST = 1.0
W, H, FX = 640, 480, 554.25


def frame(dims, voxel, centre, stride):
    """(view, depth): the camera at the grid's centre (off the nodes) looking along +x, slightly turned; the
    depth of a box room 0.3 m inside the grid's faces and a pillar 60 % of the way to the far wall."""
    half = 0.5 * voxel * (np.asarray(dims) - 1) - 0.3
    pos = np.asarray(centre, np.float64) + [0.013, -0.021, 0.017]
    quat = np.array([0.52, -0.49, 0.5, -0.51])   # optical z on world x, x (right) on -y, y (down) on -z, a little off
    view = DepthView(W, H, FX, FX, 320.5, 240.5, tuple(pos), tuple(quat), 0.1, min(5.0, 1.1 * float(half[0])), stride, True)
    x, y, z, w = quat / np.linalg.norm(quat)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ray = np.stack([(ii - view.cx) / FX, (jj - view.cy) / FX, np.ones(ii.shape)], -1) @ R.T   # per unit of depth
    rel = pos - np.asarray(centre)
    with np.errstate(divide="ignore"):
        t = np.where(ray > 0, (half - rel) / ray, (-half - rel) / ray)   # the room's faces
    depth = t.min(-1)
    # a pillar (vertical cylinder, radius 0.15 m) ahead of the camera
    c = rel[:2] - np.array([0.6 * half[0], 0.1])
    a, b, cc = (ray[..., :2] ** 2).sum(-1), 2.0 * (ray[..., :2] * c).sum(-1), float(c @ c) - 0.15 ** 2
    disc = b * b - 4.0 * a * cc
    tp = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a), np.inf)
    depth = np.where((tp > 0) & (tp < depth), tp, depth)
    depth = depth.astype(np.float32)
    depth[::37, ::11] = np.nan   # drop-outs
    return view, depth


def main():
    passes = len(sys.argv) > 1 and sys.argv[1] == "--passes"
    reps = int(sys.argv[2]) if passes and len(sys.argv) > 2 else int(sys.argv[1]) if len(sys.argv) > 1 and not passes else 30
    centre = np.asarray(STATE["arm"][:3], np.float64) + [0.0, 0.0, 0.4]
    for dims, voxel in GRIDS:
        origin = tuple(centre - 0.5 * voxel * (np.asarray(dims) - 1))
        field = DistanceField(dims, voxel, origin)
        e = Engine(make_config("arm", n_samples=4096, n_horizon=32, state_f64=True), scene=Scene(BODY), field=field)
        e.set_target([0.1, 0.4, 1.6], [-0.5, -0.5, 0.5, -0.5])
        e.set_state(np.array(STATE["arm"], np.float64)[None])
        empty = np.zeros(field.shape, np.uint8)
        for stride in STRIDES:
            view, depth = frame(dims, voxel, centre, stride)
            if passes:
                for _ in range(reps):
                    e.integrate_depth(depth, view, max_dist=MAX_DIST)
                e.synchronize()
                print(f"{dims} stride {stride}: {reps} integrate_depth calls")
                continue
            t_host = []
            for _ in range(3):
                t0 = time.perf_counter()
                want = depth_integrate_host(field, empty, depth, view)
                t_host.append(time.perf_counter() - t0)
            e.set_occupancy(empty)
            e.integrate_depth(depth, view, max_dist=MAX_DIST)
            got = e.get_occupancy()
            assert np.array_equal(got, want), "device map differs from the host twin's"
            t_depth, t_occ = [], []
            for i in range(reps + 5):
                t0 = time.perf_counter()
                e.integrate_depth(depth, view, max_dist=MAX_DIST)
                e.synchronize()
                t1 = time.perf_counter()
                e.set_occupancy(got, max_dist=MAX_DIST)
                e.synchronize()
                t2 = time.perf_counter()
                if i >= 5:
                    t_depth.append(t1 - t0)
                    t_occ.append(t2 - t1)
            assert np.array_equal(e.get_occupancy(), want)
            print(f"{dims[0]}x{dims[1]}x{dims[2]} voxel {voxel} frame {W}x{H} stride {stride} max_dist {MAX_DIST} "
                  f"({int(want.sum())} nodes occupied, {int(np.isfinite(depth).sum())} finite pixels), {reps} reps")
            print(f"  depth (us)       {stats(t_depth)}")
            print(f"  occupancy (us)   {stats(t_occ)}")
            print(f"  host cast (ms)   {stats(t_host, 1e3)}")
            e.run_steps(3)   # and the controller goes on with the field in place
            e.synchronize()
        e.close()


if __name__ == "__main__":
    main()
