#!/usr/bin/env python3
"""rm_slice_mesh on two device-resident meshes, by turns in one process: an icosphere of 20 * 4^level triangles and the marching-cubes
mesh of a scene from extract_mesh (as tools/voxel_probe.py builds them), each in 256 and in 1024 layers across z.  Wall-clock host to
host around the synchronous call (the read of the slices into device tensors included); prints median / fastest / slowest, counts and
stats.  Beside them for scale: rm_slice_contours of the scene at 1024 x 1024 points per layer over the same planes, the write
bandwidth rm_measure_write_bandwidth reports, and the time the bytes each kernel family of one call has to move (a model from the
counts, written out below) would take at that bandwidth.

  python tools/mesh_slice_probe.py --resolution 256 --level 8 --reps 9 --warmup 2"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from ray_marching_amd import _ffi, csg, renderer  # noqa: E402
from voxel_probe import icosphere  # noqa: E402


def model_bytes(n_vertices, counts, stats, n_layers):
    """Bytes each kernel family of one rm_slice_mesh call reads and writes at the least (every array once per launch that touches it;
    the gathers of snapped corners and of neighbours' states counted as if they were streams)."""
    H, N, C = 3 * counts["triangles"], counts["points"], counts["contours"]
    edge_bits = max(1, 2 * max(0, int(n_vertices - 1).bit_length()))
    edge_passes = (edge_bits + 7) // 8
    item_passes = stats["sort_passes"] - edge_passes
    rounds = stats["rank_rounds"]
    return {
        "snap": n_vertices * 24,
        "keys": H * (4 + 12 + 12),
        "edge sort": edge_passes * H * (8 + 12 + 12),
        "groups + count + scan": H * (12 + 4 + 4) + H * (4 + 4 + 12 + 8) + H * 8,
        "items": N * (12 + 8),
        "item sort": item_passes * N * (8 + 12 + 12),
        "ids + link": N * (12 + 8) + N * (12 + 2 * (12 + 12 + 8) + 8),
        "ranking": N * (4 + 8) + 2 * rounds * N * (8 + 8 + 8) + N * (8 + 4 + 4 + 8),
        "contours": N * (4 + 4) * 2 + N * (8 + 4 + 4) + C * 16,
        "emit": N * (12 + 2 * 12 + 8 + 4 + 12 + 4) + C * 16,
    }


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32")
    ap.add_argument("--resolution", type=int, default=256, help="lattice of the scene's mesh, and the icosphere's size in steps")
    ap.add_argument("--level", type=int, default=8, help="subdivisions of the icosphere: 20 * 4^level triangles")
    ap.add_argument("--layers", default="256,1024")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-contours", action="store_true", help="leave rm_slice_contours and the bandwidth out (a profiler run)")
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
    times, result = {name: [] for name in jobs}, {}
    for r in range(a.warmup + a.reps):
        for name, (vv, tt, o, s, h) in jobs.items():
            t0 = time.perf_counter()
            result[name] = res.slice_mesh(vv, tt, o, s, 2, heights=h, device=True)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if r >= a.warmup:
                times[name].append(dt * 1e3)
    print("resolution %d, icosphere level %d, scene %s, %d reps after %d warm-up rounds, alternating" % (n, a.level, a.scene, a.reps, a.warmup))
    for name, ts in times.items():
        print("%-28s median %9.3f ms  fastest %9.3f ms  slowest %9.3f ms" % (name, statistics.median(ts), min(ts), max(ts)))
    for name, s in result.items():
        print("%s: counts %s" % (name, s.counts))
        print("%s: stats %s" % (name, s.stats))
    if not a.no_contours:
        gbps = res.measure_write_bandwidth()
        bw = gbps * 1e9
        print("write bandwidth: %.1f GB/s" % gbps)
        for name, (vv, tt, o, s, h) in jobs.items():
            mb = model_bytes(len(vv), result[name].counts, result[name].stats, len(h))
            total = sum(mb.values())
            print("%s: model %.1f MB in all = %.3f ms at the write bandwidth; per family (ms): %s"
                  % (name, total / 1e6, total / bw * 1e3, ", ".join("%s %.3f" % (k, b / bw * 1e3) for k, b in mb.items())))
        for nl in (int(x) for x in a.layers.split(",")):
            h = (-2.5 + (np.arange(nl) + 0.5) * (5.0 / nl)).astype(np.float32)
            ts = []
            for r in range(a.warmup + 3):
                t0 = time.perf_counter()
                c = res.slice_contours((-2.5,) * 3, (2.5,) * 3, 1024, heights=h, axis=2, device=True)
                torch.cuda.synchronize()
                if r >= a.warmup:
                    ts.append((time.perf_counter() - t0) * 1e3)
            print("rm_slice_contours of %s, 1024 x 1024, %d layers: median %9.3f ms (%d points, %d contours)"
                  % (a.scene, nl, statistics.median(ts), len(c.points), len(c.contours)))
    res.close()


if __name__ == "__main__":
    main()
