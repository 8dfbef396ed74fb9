#!/usr/bin/env python3
"""Mesh-export throughput on one GPU (rm_sample_grid, rm_extract_mesh); prints one JSON line.

  sample_grid:  512^3 lattice (2^27 points), g32 over [-2.5, 2.5]^3 and mat_mix over [-3, 3]^3, into a torch tensor;
                device events around each call on the caller's stream (median over --reps after --warmup calls)
  extract_mesh: g32 over [-2.5, 2.5]^3 at 512^3, host to host (the call is synchronous), without and with normals + ids;
                vertex and triangle counts, and the bytes the count / scan / emit kernels move at least, counted from the
                shapes (their kernel times come from a rocprofv3 --kernel-trace --stats run of this probe)
  sparse:       rm_extract_mesh_sparse on the same lattice, host to host, alternating with the dense call in one loop
                (median, fastest and slowest of each over --reps rounds), with its statistics; with --big also g32 at
                1281^3 (step 2^-8) and 2561^3 (step 2^-9) from origin -2.5, which the dense call cannot hold

usage: tools/mesh_probe.py [--reps N] [--res N] [--big] > profiles/r08_sparse_mesh.txt"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ray_marching_amd import csg, mesh, renderer  # noqa: E402


def timed(torch, fn, warmup, reps):
    """Median device time (ms) of fn() on the current stream."""
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def host_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def lattice(lo, hi, n):
    step = (np.float32(hi) - np.float32(lo)) / np.float32(n - 1)
    return (lo,) * 3, (float(step),) * 3, (n, n, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--big", action="store_true", help="also time the sparse extraction at 1281^3 and 2561^3")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream  # noqa: E731
    res = renderer.RayMarchingResources(0)
    res.set_materials(mesh.MATERIALS)
    res.set_limits(renderer.RayMarchLimits(0.01, 100.0, 256))
    n = a.res
    pts = n ** 3
    out = {"lattice": [n, n, n], "points": pts, "gpu": torch.cuda.get_device_name(dev)}
    d = torch.empty(pts, dtype=torch.float32, device=dev)
    for scene, lo, hi in (("g32", -2.5, 2.5), ("mat_mix", -3.0, 3.0)):
        res.set_scene(csg.scene(scene))
        o, s, shape = lattice(lo, hi, n)
        t = timed(torch, lambda: res.sample_grid_device(o, s, shape, d.data_ptr(), stream=stream()), a.warmup, a.reps)
        out["sample_%s_ms" % scene] = round(t, 4)
        out["sample_%s_gpts_per_s" % scene] = round(pts / t / 1e6, 2)
    del d
    res.set_scene(csg.scene("g32"))
    o, s, shape = lattice(-2.5, 2.5, n)
    m = res.extract_mesh_grid(o, s, shape, normals=False, ids=False)
    V, T = len(m.vertices), len(m.triangles)
    L, h = res._L, res._h
    import ctypes as C
    fo, fs = (C.c_float * 3)(*o), (C.c_float * 3)(*s)
    counts = (C.c_uint64 * 2)()
    for label, flags in (("plain", 0), ("attrs", 3)):
        out["extract_%s_host_ms" % label] = round(host_ms(lambda: L.rm_extract_mesh(h, fo, fs, n, n, n, 0.0, flags, counts),
                                                          a.warmup, a.reps), 4)
    blocks = (pts + 2047) // 2048
    # least bytes of count (dist), scan (block sums), vertex emit (dist; vbase, flags, vertices) and triangle emit (flags of
    # the cells' corners once; triangles): the distances are read twice, the flags written once and read once
    out.update({"vertices": V, "triangles": T, "closed": m.is_closed(),
                "extract_kernel_bytes": 4 * pts + 16 * blocks + (4 + 4 + 1) * pts + 12 * V + pts + 12 * T})
    # dense and sparse by turns, so that both see the same state of the machine
    stats = (C.c_uint64 * 6)()
    dense = lambda: L.rm_extract_mesh(h, fo, fs, n, n, n, 0.0, 0, counts)  # noqa: E731
    sparse = lambda: L.rm_extract_mesh_sparse(h, fo, fs, n, n, n, 0.0, 0, stats, 6)  # noqa: E731
    for _ in range(a.warmup):
        assert dense() == 0 and sparse() == 0
    td, ts = [], []
    for _ in range(a.reps):
        for fn, t in ((dense, td), (sparse, ts)):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
    names = ("vertices", "triangles", "bricks", "bricks_kept", "evaluations", "scratch_bytes")
    for label, t in (("dense", td), ("sparse", ts)):
        out["ab_%s_host_ms" % label] = {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    out["sparse_stats"] = {k: int(stats[i]) for i, k in enumerate(names)}
    out["sparse_evaluations_per_vertex"] = round(int(stats[4]) / max(int(stats[0]), 1), 2)
    out["sparse_matches_dense_counts"] = int(stats[0]) == V and int(stats[1]) == T
    if a.big:
        for big, step in ((1281, 2.0 ** -8), (2561, 2.0 ** -9)):
            bo, bs = (C.c_float * 3)(-2.5, -2.5, -2.5), (C.c_float * 3)(step, step, step)
            run = lambda: L.rm_extract_mesh_sparse(h, bo, bs, big, big, big, 0.0, 0, stats, 6)  # noqa: E731
            rc = run()
            if rc != 0:
                out["sparse_%d" % big] = {"status": rc}
                continue
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                run()
                t.append((time.perf_counter() - t0) * 1e3)
            row = {k: int(stats[i]) for i, k in enumerate(names)}
            row.update({"host_ms": round(float(np.median(t)), 3), "evaluations_per_vertex": round(int(stats[4]) / max(int(stats[0]), 1), 2)})
            out["sparse_%d" % big] = row
    res.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
