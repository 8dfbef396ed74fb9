#!/usr/bin/env python3
"""rm_label_solid against the first step of the only earlier route to the same answer, rm_sample_grid on the same lattice
(device output: no copy to the host, no labelling there), alternating in one process.  Prints median / fastest / slowest of
each, the call's counts and its stats (MERGE_PASSES among them).

  python tools/topology_probe.py --scene g32 --resolution 256 --reps 15 --warmup 3"""
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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    res = renderer.RayMarchingResources(0)
    res.set_scene(csg.scene(a.scene))
    lo, step, n = res._box_lattice(a.lo, a.hi, a.resolution)
    shape = tuple(int(x) for x in n)
    out = torch.empty(shape[0] * shape[1] * shape[2], dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream()

    def grid():
        res.sample_grid(lo, step, shape, out=out)
        stream.synchronize()

    result = []

    def label():
        result[:] = [res.label_solid_grid(lo, step, shape, a.level)]   # synchronous; reads both row tables back

    times = {"rm_label_solid": [], "rm_sample_grid": []}
    for r in range(a.warmup + a.reps):
        for name, fn in (("rm_label_solid", label), ("rm_sample_grid", grid)):
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if r >= a.warmup:
                times[name].append(dt * 1e3)
    print("scene %s, %dx%dx%d over [%g, %g]^3, level %g, %d reps after %d warm-up rounds, alternating"
          % (a.scene, shape[0], shape[1], shape[2], a.lo, a.hi, a.level, a.reps, a.warmup))
    for name, t in times.items():
        print("%-16s median %8.3f ms  fastest %8.3f ms  slowest %8.3f ms" % (name, statistics.median(t), min(t), max(t)))
    t = result[0]
    print("counts:", t.counts)
    print("stats:", t.stats)
    res.close()


if __name__ == "__main__":
    main()
