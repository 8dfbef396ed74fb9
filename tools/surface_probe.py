#!/usr/bin/env python3
"""rm_surface_solid of a scene and rm_surface_classes of random 8-class bytes (a device tensor: no copy from the host) at 128^3,
256^3 and 512^3 points.  Prints median / fastest / slowest of each call, and the bytes per second the median amounts to against
ONE read of the lattice (one byte per point) -- beside the HBM figures of the MI355X: 8.0 TB/s peak, 6.29 TB/s measured for a
float4 copy.  The call is more than the count kernel: the front end's copy of the caller's bytes (a solid: probe, scan and
occupancy kernels), rm_surf_count_kernel, rm_surf_reduce_kernel, 6.7 KB back to the host and a synchronisation.  The kernels' own
times come from a rocprofv3 --kernel-trace --stats run of this probe.

  python tools/surface_probe.py --scene g32 --reps 11 --warmup 2"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from ray_marching_amd import csg, renderer  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32")
    ap.add_argument("--lo", type=float, default=-2.5)
    ap.add_argument("--hi", type=float, default=2.5)
    ap.add_argument("--resolutions", default="128,256,512")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)
    res = renderer.RayMarchingResources(0)
    res.set_scene(csg.scene(a.scene))
    print("scene %s over [%g, %g]^3 and random 8-class bytes, %d reps after %d warm-up rounds, alternating" % (a.scene, a.lo, a.hi, a.reps, a.warmup))
    print("HBM: %.1f TB/s peak, %.2f TB/s measured for a float4 copy" % (HBM_PEAK / 1e12, HBM_COPY / 1e12))
    for n in (int(x) for x in a.resolutions.split(",")):
        lo, step, shape = res._box_lattice(a.lo, a.hi, n)
        shape = tuple(int(x) for x in shape)
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(n)
        classes = torch.randint(0, 8, (n, n, n), dtype=torch.uint8, device="cuda:0", generator=gen)
        torch.cuda.synchronize()
        result = {}

        def solid():
            result["solid"] = res.surface_solid_grid(lo, step, shape, 0.0)

        def random_classes():
            result["classes"] = res.surface_classes(classes)

        times = {"rm_surface_solid": [], "rm_surface_classes": []}
        for r in range(a.warmup + a.reps):
            for name, fn in (("rm_surface_solid", solid), ("rm_surface_classes", random_classes)):
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if r >= a.warmup:
                    times[name].append(dt * 1e3)
        print("%d^3 points (%.1f MB of classes)" % (n, n ** 3 / 1e6))
        for name, t in times.items():
            med = statistics.median(t)
            rate = n ** 3 / (med * 1e-3)
            print("  %-19s median %8.3f ms  fastest %8.3f ms  slowest %8.3f ms  %7.1f GB/s of one read (%.1f %% of the peak)"
                  % (name, med, min(t), max(t), rate / 1e9, 100.0 * rate / HBM_PEAK))
        s, c = result["solid"], result["classes"]
        print("  solid: area %.6f, facet area %.6f, points %d, stats %s" % (s.measures(1, 0)["area"], s.measures(1, 0)["facet_area"], int(s.points[1]), s.stats))
        print("  classes: points %s, scratch %d bytes" % (" ".join(str(int(x)) for x in c.points), c.stats["scratch_bytes"]))
        del classes
    res.close()


if __name__ == "__main__":
    main()
