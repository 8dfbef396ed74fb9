#!/usr/bin/env python3
"""Whole 1080p rm_draw_lattice calls into device memory, one process per library: the voxelised extract_mesh of a scene at two
resolutions, a 10 % sparse lattice and a full one, and for context rm_draw of the scene's program at the same camera.  Device
events around each call on one stream; prints median / fastest / slowest per case and a checksum of the image.  The library is
the one the package loads: as built, or -- RM_HIP_SO -- a variant whose traversal visits every cell, the same device code over
brick bits that rm_set_lattice has all set (tools/ab_build.sh noskip -DRM_LAT_SKIP=0).  Run the two by turns and compare the
checksums: both must write the same bytes.

  tools/ab_build.sh noskip -DRM_LAT_SKIP=0
  python tools/lattice_draw_probe.py --reps 15 --warmup 3
  RM_HIP_SO=build/variants/librm_hip_noskip.so python tools/lattice_draw_probe.py --reps 15 --warmup 3"""
import argparse
import hashlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from ray_marching_amd import _ffi, camera, csg, renderer  # noqa: E402

def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32")
    ap.add_argument("--resolutions", default="256,512")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    W, H = (int(x) for x in a.size.split("x"))
    dev = torch.device("cuda", 0)
    res = renderer.RayMarchingResources(0)
    res.set_scene(csg.scene(a.scene))
    palette = [[0.4, 0.7, 0.1], [0.72, 0.72, 0.75], [0.9, 0.15, 0.1]]
    ctl = camera.OrbitCameraController.new([0.0, 0.0, 0.0], 6.0)
    ctl.update(camera.Orbit([35.0, -25.0]))
    u = renderer.prepare_uniforms((W, H), ctl.camera())
    libs = {os.path.basename(_ffi.HIP_SO): res}
    for lib in libs.values():
        lib.set_uniforms(u)
        lib.set_materials(palette)
    # the lattices, all on the device
    cases = {}
    for n in (int(x) for x in a.resolutions.split(",")):
        lo, step, shape = res._box_lattice(-2.5, 2.5, n)
        shape = tuple(int(x) for x in shape)
        m = res.extract_mesh_grid(lo, step, shape, normals=False, ids=False, device=True)
        vox = res.voxelize_mesh(m.vertices, m.triangles, lo, step, shape)
        cases["%s mesh %d^3" % (a.scene, n)] = (vox.occupancy_device().clone(), lo, step, vox.counts["inside"])
        del m
    n = int(a.resolutions.split(",")[0])
    lo, step, shape = res._box_lattice(-2.5, 2.5, n)
    g = torch.Generator(device=dev).manual_seed(28)
    sparse = (torch.rand((n, n, n), device=dev, generator=g) < 0.1).to(torch.uint8)
    cases["10 %% sparse %d^3" % n] = (sparse, lo, step, int(sparse.sum()))
    cases["full %d^3" % n] = (torch.ones((n, n, n), dtype=torch.uint8, device=dev), lo, step, n ** 3)
    out = {name: torch.empty((H, W, 4), dtype=torch.float32, device=dev) for name in libs}
    stream = torch.cuda.current_stream(dev).cuda_stream
    times = {}
    print("%dx%d, device destination, %d reps after %d warm-up rounds" % (W, H, a.reps, a.warmup))
    for case, (cls, lo, step, points) in cases.items():
        for name, lib in libs.items():
            lib.set_lattice(cls, lo, step)
        for r in range(a.warmup + a.reps):
            for name, lib in libs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                lib.draw_lattice_device(W, H, out[name].data_ptr(), stream=stream)
                e1.record()
                e1.synchronize()
                if r >= a.warmup:
                    times.setdefault((case, name), []).append(e0.elapsed_time(e1))
        for name in libs:
            ts = times[(case, name)]
            digest = hashlib.sha256(out[name].cpu().numpy().tobytes()).hexdigest()[:16]
            print("%-18s %-22s median %8.3f ms  fastest %8.3f ms  slowest %8.3f ms  (%d points; image %s)"
                  % (case, name, statistics.median(ts), min(ts), max(ts), points, digest))
    # for context: rm_draw of the program at the same camera
    res.set_limits(renderer.RayMarchLimits(0.01, 100.0, 128))
    ts = []
    for r in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res.draw_device(W, H, next(iter(out.values())).data_ptr(), stream=stream)
        e1.record()
        e1.synchronize()
        if r >= a.warmup:
            ts.append(e0.elapsed_time(e1))
    print("%-18s %-22s median %8.3f ms  fastest %8.3f ms  slowest %8.3f ms" % ("rm_draw " + a.scene, next(iter(libs)), statistics.median(ts), min(ts), max(ts)))
    for lib in libs.values():
        lib.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
