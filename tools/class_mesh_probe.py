#!/usr/bin/env python3
"""rm_mesh_classes of three class lattices on the device (no copy from the host): a ball at 256^3, the support mask of a
voxelised torus mesh at 256^3 (classes 3 and 4 against the rest) and a checkerboard at 128^3 (the worst case: every pair of
neighbours is a face).  Prints median / fastest / slowest of each call and, beside it, the time the call's own bytes would take at
the figure rm_measure_write_bandwidth reports on this machine: the copy of the caller's bytes (n read, n written), the mark
kernel (n read, 12 bytes per word of 64 corners written), the emit kernel (n and those 12 bytes per word read, the mesh written:
12 bytes per vertex, 20 per triangle).  For scale: rm_surface_classes of the same bytes and rm_extract_mesh of a scene on a lattice
of the same size, on the device.  The kernels' own times come from a rocprofv3 --kernel-trace --stats run of this probe with
one --input.

  python tools/class_mesh_probe.py --reps 7 --warmup 2
  rocprofv3 --kernel-trace --stats -- python tools/class_mesh_probe.py --input checker --reps 3 --warmup 1"""
import argparse
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ray_marching_amd import csg, renderer  # noqa: E402

INPUTS = ("ball", "supports", "checker")


def torus_mesh(nu, nv, R, r, centre):
    """A torus around the y axis (so that its upper half overhangs for +z): vertices (nu nv, 3) float32, triangles uint32."""
    u, v = np.meshgrid(np.arange(nu) * (2.0 * math.pi / nu), np.arange(nv) * (2.0 * math.pi / nv), indexing="ij")
    ring = R + r * np.cos(v)
    xyz = np.stack([ring * np.cos(u), r * np.sin(v), ring * np.sin(u)], axis=-1).reshape(-1, 3) + np.asarray(centre)
    a = (np.arange(nu)[:, None] * nv + np.arange(nv)[None, :]).reshape(-1)
    b = (((np.arange(nu) + 1) % nu)[:, None] * nv + np.arange(nv)[None, :]).reshape(-1)
    c = (((np.arange(nu) + 1) % nu)[:, None] * nv + ((np.arange(nv) + 1) % nv)[None, :]).reshape(-1)
    d = (np.arange(nu)[:, None] * nv + ((np.arange(nv) + 1) % nv)[None, :]).reshape(-1)
    return xyz.astype(np.float32), np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)]).astype(np.uint32)


def lattice(res, name):
    """(classes on the device, the class set to mesh, n per axis)."""
    dev = torch.device("cuda", res.device)
    if name == "ball":
        n = 256
        x = torch.arange(n, device=dev, dtype=torch.float32) - 127.3
        d2 = x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2
        return (d2 < 100.4 ** 2).to(torch.uint8).contiguous(), (1,), n
    if name == "checker":
        n = 128
        i = torch.arange(n, device=dev)
        return ((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2 == 0).to(torch.uint8).contiguous(), (1,), n
    n = 256
    v, t = torus_mesh(256, 128, 80.0, 30.0, (127.5, 127.5, 127.5))
    vox = res.voxelize_mesh(v, t, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (n, n, n))
    sup = res.support_occupancy(vox.occupancy_device(), up="+z", r2=1)
    mask = torch.empty((n, n, n), dtype=torch.uint8, device=dev)
    res.read_support_device(mask_ptr=mask.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return mask, (3, 4), n


def timed(fn, reps, warmup):
    t = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--input", default="all", choices=INPUTS + ("all",))
    ap.add_argument("--scene", default="g32", help="the scene of the rm_extract_mesh comparison")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)
    res = renderer.RayMarchingResources(0)
    res.set_scene(csg.scene(a.scene))
    gbps = res.measure_write_bandwidth()
    print("rm_measure_write_bandwidth: %.1f GB/s; %d reps after %d warm-up rounds" % (gbps, a.reps, a.warmup))
    for name in (INPUTS if a.input == "all" else (a.input,)):
        classes, members, n = lattice(res, name)
        result = {}

        def mesh_classes():
            result["mesh"] = res.mesh_classes(classes, members, device=True)

        def surface_classes():
            result["surface"] = res.surface_classes(classes)

        def extract_mesh():
            lo, step, shape = res._box_lattice(-2.5, 2.5, n)
            result["extract"] = res.extract_mesh_grid(lo, step, tuple(int(x) for x in shape), normals=False, ids=False, device=True)

        rows = [(label, timed(fn, a.reps, a.warmup)) for label, fn in (("rm_mesh_classes + read", mesh_classes), ("rm_surface_classes", surface_classes),
                                                                         ("rm_extract_mesh + read", extract_mesh))]
        m = result["mesh"]
        points, words = n ** 3, ((n + 64) // 64) * (n + 1) ** 2
        own = 2 * points + (points + 12 * words) + (points + 12 * words + 12 * m.counts["vertices"] + 20 * m.counts["triangles"])
        floor_ms = own / (gbps * 1e9) * 1e3
        print("%s: %d^3 points, classes %s against the rest: %s" % (name, n, list(members), m.counts))
        print("  retained %d bytes, scratch %d bytes; own bytes %d = %.3f ms at %.1f GB/s" % (m.stats["retained_bytes"], m.stats["scratch_bytes"], own, floor_ms, gbps))
        for label, (med, lo_, hi_) in rows:
            print("  %-24s median %9.3f ms  fastest %9.3f ms  slowest %9.3f ms" % (label, med, lo_, hi_))
        e = result["extract"]
        print("  (rm_extract_mesh of %s: %d vertices, %d triangles)" % (a.scene, len(e.vertices), len(e.triangles)))
        del classes, result
    res.close()


if __name__ == "__main__":
    main()
