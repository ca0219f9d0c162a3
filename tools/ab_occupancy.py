"""What a map change costs: the field built on the device from the occupancy bytes (Engine.set_occupancy)
against the route without it -- a Euclidean distance transform on the host, then set_distance_field --
for the same map, in the same process (tools/, not shipped).

    python tools/ab_occupancy.py [reps]          the table
    python tools/ab_occupancy.py --passes [n]    n set_occupancy calls per case and nothing else: the run to
                                                 put under a kernel trace for the per-pass times

Per grid (64^3, 128^3, 512 x 64 x 64; a floor under the grid's centre and a box beside it, as
tools/ab_distance_field.py's world) and per max_dist (None, 1 m), wall time around work that ends in a
synchronise, after 5 warm-up calls of each, alternating the two device routes call by call:
  occupancy   set_occupancy(occ) + synchronize: the bytes' copy, the four launches, the header
  upload      set_distance_field(d) + synchronize on a finished field: host packing and the 8 B / node copy
              -- the whole of the other route's device side, and the bar the occupancy path has to come under
  host EDT    the transform the other route needs first: scipy.ndimage.distance_transform_edt twice (to the
              occupied and to the free nodes) and the signed combination, where scipy is installed; and the
              library's own host helper (mppi_occupancy_field) for the same map
Medians and interquartile ranges in microseconds (host EDT: milliseconds, 3 runs).  The device field is
compared with the host helper's bit for bit before anything is timed.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from quadrotor_manipulator_mppi_amd.engine import DistanceField, Engine, Scene, make_config
from tools.ab_native import STATE
from tools.ab_obstacles import BODY

GRIDS = [((64, 64, 64), 2.0 / 63), ((128, 128, 128), 2.0 / 127), ((512, 64, 64), 0.03)]
CAPS = [None, 1.0]


def world(dims, voxel, centre):
    c = np.asarray(centre, np.float64)
    origin = c - 0.5 * voxel * (np.asarray(dims) - 1)
    boxes = [((-99.0, -99.0, -99.0), (99.0, 99.0, c[2] - 0.6)), (tuple(c + [0.3, -0.2, -0.3]), tuple(c + [0.6, 0.2, 0.4]))]
    return DistanceField.from_boxes(boxes, dims, voxel, origin)


def scipy_route(occ, voxel, cap):
    from scipy import ndimage
    to_occ = ndimage.distance_transform_edt(~occ)
    to_free = ndimage.distance_transform_edt(occ)
    d = voxel * np.where(occ, -(to_free - 0.5), to_occ - 0.5)
    return np.clip(d, -cap, cap).astype(np.float32) if cap else d.astype(np.float32)


def stats(ts, scale=1e6):
    ts = np.asarray(ts) * scale
    q1, q3 = np.percentile(ts, [25, 75])
    return f"{np.median(ts):9.1f} (IQR {q3 - q1:6.1f}, min {ts.min():9.1f})"


def main():
    passes = len(sys.argv) > 1 and sys.argv[1] == "--passes"
    reps = int(sys.argv[2]) if passes and len(sys.argv) > 2 else int(sys.argv[1]) if len(sys.argv) > 1 and not passes else 30
    centre = np.asarray(STATE["arm"][:3], np.float64) + [0.0, 0.0, 0.4]
    for dims, voxel in GRIDS:
        f = world(dims, voxel, centre)
        occ = f.d < 0.0
        e = Engine(make_config("arm", n_samples=4096, n_horizon=32, state_f64=True), scene=Scene(BODY),
                   field=DistanceField(f.dims, f.voxel, f.origin))
        e.set_target([0.1, 0.4, 1.6], [-0.5, -0.5, 0.5, -0.5])
        e.set_state(np.array(STATE["arm"], np.float64)[None])
        for cap in CAPS:
            if passes:
                for _ in range(reps):
                    e.set_occupancy(occ, max_dist=cap)
                e.synchronize()
                print(f"{dims} max_dist {cap}: {reps} set_occupancy calls")
                continue
            host = DistanceField.from_occupancy(occ, f.dims, f.voxel, f.origin, cap).d
            e.set_occupancy(occ, max_dist=cap)
            dev = e.get_distance_field()[0]
            assert np.array_equal(dev.view(np.uint32), host.view(np.uint32)), "device field differs from the host helper's"
            t_occ, t_up = [], []
            for i in range(reps + 5):
                t0 = time.perf_counter()
                e.set_occupancy(occ, max_dist=cap)
                e.synchronize()
                t1 = time.perf_counter()
                e.set_distance_field(host)
                e.synchronize()
                t2 = time.perf_counter()
                if i >= 5:
                    t_occ.append(t1 - t0)
                    t_up.append(t2 - t1)
            t_helper, t_scipy = [], []
            for _ in range(3):
                t0 = time.perf_counter()
                DistanceField.from_occupancy(occ, f.dims, f.voxel, f.origin, cap)
                t_helper.append(time.perf_counter() - t0)
            try:
                for _ in range(3):
                    t0 = time.perf_counter()
                    scipy_route(occ, f.voxel, cap)
                    t_scipy.append(time.perf_counter() - t0)
            except ImportError:
                pass
            print(f"{dims[0]}x{dims[1]}x{dims[2]} voxel {voxel:.4f} max_dist {cap} ({int(occ.sum())} of {occ.size} nodes occupied), {reps} reps")
            print(f"  occupancy (us)      {stats(t_occ)}")
            print(f"  upload (us)         {stats(t_up)}")
            print(f"  host EDT, scipy (ms) {stats(t_scipy, 1e3) if t_scipy else 'not measured (no scipy)'}")
            print(f"  host EDT, helper (ms){stats(t_helper, 1e3)}")
            e.run_steps(3)   # and the controller goes on with the field in place
            e.synchronize()
        e.close()


if __name__ == "__main__":
    main()
