#!/usr/bin/env python3
"""rm_hatch_slices on the slices of the two device-resident meshes of tools/mesh_slice_probe.py (an icosphere of 20 * 4^level
triangles and the marching-cubes mesh of a scene, each in 256 and in 1024 layers across z), by turns in one process: every round
slices a mesh (rm_slice_mesh, timed as there) and then hatches the retained slices at a spacing that gives about --lines lines per
layer, 45 degrees, turning 90 degrees per layer.  Wall-clock host to host around the synchronous call, the read of the hatch into
device tensors included; prints median / fastest / slowest of both calls, counts and stats.  Beside them for scale: the write
bandwidth rm_measure_write_bandwidth reports, and the time the bytes each kernel family of one hatch has to move (a model from the
counts, written out below) would take at that bandwidth.

  python tools/hatch_probe.py --resolution 256 --level 8 --reps 9 --warmup 2"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from ray_marching_amd import csg, renderer, slicer  # noqa: E402
from voxel_probe import icosphere  # noqa: E402


def model_bytes(n_points, counts, stats):
    """Bytes each kernel family of one rm_hatch_slices call reads and writes at the least (every array once per launch that touches
    it; the binary searches and the gathers of points counted as if they were streams)."""
    P, N, H = n_points, counts["crossings"], counts["segments"]
    return {
        "count": P * (12 + 12 + 16 + 4 + 4),
        "scans": P * 8 + N * 8,
        "items": N * (4 + 4 + 12 + 12 + 16 + 8 + 4 + 8),
        "sort": stats["sort_passes"] * N * (8 + 12 + 12),
        "pair": N * (8 + 8 + 4),
        "emit": N * (8 + 4 + 4 + 4) + H * (8 + 8 + 16 + 4),
    }


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32")
    ap.add_argument("--resolution", type=int, default=256, help="lattice of the scene's mesh, and the icosphere's size in steps")
    ap.add_argument("--level", type=int, default=8, help="subdivisions of the icosphere: 20 * 4^level triangles")
    ap.add_argument("--layers", default="256,1024")
    ap.add_argument("--lines", type=int, default=500, help="lines per layer the spacing aims at")
    ap.add_argument("--zigzag", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-bandwidth", action="store_true", help="leave the bandwidth and the model out (a profiler run)")
    a = ap.parse_args(argv)
    n = a.resolution
    res = renderer.RayMarchingResources(0)
    res.set_scene(csg.scene(a.scene))
    dev = torch.device("cuda", 0)
    lo, step, shape = res._box_lattice(-2.5, 2.5, n)
    v, t = icosphere(a.level, 0.4 * n, ((n - 1) / 2.0 + 0.25,) * 3)
    m = res.extract_mesh_grid(lo, step, tuple(int(x) for x in shape), normals=False, ids=False, device=True)
    meshes = {"icosphere": (torch.from_numpy(v).to(dev), torch.from_numpy(t.view(np.int32)).to(dev), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0),
                            (0.1 * n, 0.9 * n)),
              a.scene + " mesh": (m.vertices, m.triangles, lo, step, (-2.5, 2.5))}
    jobs = {}
    for name, (vv, tt, o, s, (z0, z1)) in meshes.items():
        for nl in (int(x) for x in a.layers.split(",")):
            h = (z0 + (np.arange(nl) + 0.5) * ((z1 - z0) / nl)).astype(np.float32)
            jobs["%s, %d layers" % (name, nl)] = (vv, tt, o, s, h)
    torch.cuda.synchronize()
    slice_ms, hatch_ms = {name: [] for name in jobs}, {name: [] for name in jobs}
    result, sliced, lines = {}, {}, {}
    for r in range(a.warmup + a.reps):
        for name, (vv, tt, o, s, h) in jobs.items():
            t0 = time.perf_counter()
            sliced[name] = res.slice_mesh(vv, tt, o, s, 2, heights=h, device=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if name not in lines:       # once, outside the timed part: the extent of the points on the host
                g = sliced[name].numpy()
                extent = g.points[:, :2].max(axis=0) - g.points[:, :2].min(axis=0)
                lines[name] = slicer.hatch_lines(g, float(np.hypot(*extent)) / a.lines, 45.0, 90.0)
                t1 = time.perf_counter()
            result[name] = res.hatch_slices(lines[name][0], lines[name][1], zigzag=a.zigzag, device=True)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if r >= a.warmup:
                slice_ms[name].append((t1 - t0) * 1e3)
                hatch_ms[name].append((t2 - t1) * 1e3)
    print("resolution %d, icosphere level %d, scene %s, about %d lines per layer, %d reps after %d warm-up rounds, alternating"
          % (n, a.level, a.scene, a.lines, a.reps, a.warmup))
    for name in jobs:
        ts, hs = slice_ms[name], hatch_ms[name]     # (the lines are chosen in the first round: keep --warmup >= 1)
        print("%-28s rm_slice_mesh median %9.3f ms | rm_hatch_slices median %9.3f ms  fastest %9.3f ms  slowest %9.3f ms  (%d lines)"
              % (name, statistics.median(ts), statistics.median(hs), min(hs), max(hs), lines[name][1]))
    for name, hres in result.items():
        print("%s: %d points; counts %s" % (name, len(sliced[name].points), hres.counts))
        print("%s: stats %s" % (name, hres.stats))
    if not a.no_bandwidth:
        gbps = res.measure_write_bandwidth()
        bw = gbps * 1e9
        print("write bandwidth: %.1f GB/s" % gbps)
        for name in jobs:
            mb = model_bytes(len(sliced[name].points), result[name].counts, result[name].stats)
            total = sum(mb.values())
            print("%s: model %.1f MB in all = %.3f ms at the write bandwidth; per family (ms): %s"
                  % (name, total / 1e6, total / bw * 1e3, ", ".join("%s %.3f" % (k, b / bw * 1e3) for k, b in mb.items())))
    res.close()


if __name__ == "__main__":
    main()
