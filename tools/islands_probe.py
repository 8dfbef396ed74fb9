#!/usr/bin/env python3
"""rm_islands_solid for all six build directions and the two yardsticks -- rm_support_solid (up +z) and rm_label_solid, the
other passes over the same occupancy that share its bit planes and its union-find -- on the same lattice, by turns in one process.
Prints median / fastest / slowest of each and every direction's counts.

  python tools/islands_probe.py --scene g32 --resolution 256 --r2 1 --reps 15 --warmup 3"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_marching_amd import _ffi, csg, renderer  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32")
    ap.add_argument("--lo", type=float, default=-2.5)
    ap.add_argument("--hi", type=float, default=2.5)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--level", type=float, default=0.0)
    ap.add_argument("--r2", type=int, default=1)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-islands", action="store_true", help="leave the yardsticks out (for a kernel trace of the islands calls alone)")
    a = ap.parse_args(argv)
    res = renderer.RayMarchingResources(0)
    res.set_scene(csg.scene(a.scene))
    lo, step, n = res._box_lattice(a.lo, a.hi, a.resolution)
    shape = tuple(int(x) for x in n)
    result = {}

    def islands(up):
        def call():
            result[up] = res.islands_solid_grid(lo, step, shape, a.level, up=up, r2=a.r2)   # synchronous; nothing is read back
        return call

    calls = [("rm_islands_solid " + up, islands(up)) for up in _ffi.UP_NAMES]
    if not a.only_islands:
        calls += [("rm_support_solid +z", lambda: res.support_solid_grid(lo, step, shape, a.level, up="+z", r2=a.r2)),
                  ("rm_label_solid", lambda: res.label_solid_grid(lo, step, shape, a.level))]   # reads both row tables back
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
    for up in _ffi.UP_NAMES:
        print("counts %s: %s" % (up, result[up].counts))
    print("stats:", result["+z"].stats)
    res.close()


if __name__ == "__main__":
    main()
