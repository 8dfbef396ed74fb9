#!/usr/bin/env python3
"""rm_distance_solid, rm_distance_features (r2 = 16 for both halves) and the two yardsticks -- rm_label_solid, the other exact
whole-lattice pass, and rm_sample_grid (device output), the first step of any host-side route -- on the same lattice, by turns in
one process.  Prints median / fastest / slowest of each, the distance call's counts and stats and the features' counts.

  python tools/distance_probe.py --scene g32 --resolution 256 --reps 15 --warmup 3"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from ray_marching_amd import csg, renderer  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32")
    ap.add_argument("--lo", type=float, default=-2.5)
    ap.add_argument("--hi", type=float, default=2.5)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--level", type=float, default=0.0)
    ap.add_argument("--r2", type=int, default=16, help="squared radius of both halves of rm_distance_features")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    res = renderer.RayMarchingResources(0)
    res.set_scene(csg.scene(a.scene))
    lo, step, n = res._box_lattice(a.lo, a.hi, a.resolution)
    shape = tuple(int(x) for x in n)
    out = torch.empty(shape[0] * shape[1] * shape[2], dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream()
    result = {}

    def grid():
        res.sample_grid(lo, step, shape, out=out)
        stream.synchronize()

    def label():
        result["label"] = res.label_solid_grid(lo, step, shape, a.level)      # synchronous; reads both row tables back

    def distance():
        result["distance"] = res.distance_solid_grid(lo, step, shape, a.level)   # synchronous; nothing is read back

    def features():
        result["features"] = result["distance"].features(a.r2, a.r2)             # on the volume `distance` just made

    calls = (("rm_distance_solid", distance), ("rm_distance_features", features), ("rm_label_solid", label), ("rm_sample_grid", grid))
    times = {name: [] for name, _ in calls}
    for r in range(a.warmup + a.reps):
        for name, fn in calls:
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if r >= a.warmup:
                times[name].append(dt * 1e3)
    print("scene %s, %dx%dx%d over [%g, %g]^3, level %g, r2 %d, %d reps after %d warm-up rounds, alternating"
          % (a.scene, shape[0], shape[1], shape[2], a.lo, a.hi, a.level, a.r2, a.reps, a.warmup))
    for name, t in times.items():
        print("%-21s median %8.3f ms  fastest %8.3f ms  slowest %8.3f ms" % (name, statistics.median(t), min(t), max(t)))
    d = result["distance"]
    print("counts:", d.counts)
    print("stats:", d.stats)
    print("inscribed radius %.6f at point %s" % d.inscribed_radius())
    print("features:", result["features"].counts)
    res.close()


if __name__ == "__main__":
    main()
