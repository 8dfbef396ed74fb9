#!/usr/bin/env python3
"""Slicing throughput on one GPU (rm_slice_contours against rm_sample_grid over the same points); prints one JSON line.

  sample_grid:    g32 over [-2.5, 2.5]^3 on the points of the slices -- --res^2 points per layer, --layers planes across y
                  at mid-layer heights -- into a torch tensor; device events around each call (median over --reps after
                  --warmup calls).  This is evaluation alone, the yardstick.
  slice_contours: the same points through rm_slice_contours, host to host (the call is synchronous), and with the
                  rm_read_slices that copies the result out; points, contours and the ranking rounds of the fullest layer.
                  The per-kernel times come from a rocprofv3 --kernel-trace --stats run of this probe.

usage: tools/slice_probe.py [--reps N] [--res N] [--layers N] > profiles/r09_slice_contours.txt"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ray_marching_amd import _ffi, csg, renderer  # noqa: E402


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
    return {"median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--layers", type=int, default=64)
    ap.add_argument("--scene", default="g32")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream  # noqa: E731
    res = renderer.RayMarchingResources(0)
    res.set_limits(renderer.RayMarchLimits(0.01, 100.0, 256))
    res.set_scene(csg.scene(a.scene))
    n, nl, lo, hi = a.res, a.layers, np.float32(-2.5), np.float32(2.5)
    step = (hi - lo) / np.float32(n - 1)
    h = (hi - lo) / np.float32(nl)
    heights = res._layer_heights(lo, hi, h)
    assert len(heights) == nl, (len(heights), nl)
    pts = n * n * nl
    out = {"scene": a.scene, "axis": 1, "lattice": [n, n], "layers": nl, "points": pts, "gpu": torch.cuda.get_device_name(dev)}
    # evaluation alone: the regular lattice through the same points (y: origin lo + h / 2, step h)
    d = torch.empty(pts, dtype=torch.float32, device=dev)
    o, s, shape = (float(lo), float(heights[0]), float(lo)), (float(step), float(h), float(step)), (n, nl, n)
    t_eval = timed(torch, lambda: res.sample_grid_device(o, s, shape, d.data_ptr(), stream=stream()), a.warmup, a.reps)
    del d
    out["sample_grid_ms"] = round(t_eval, 3)
    out["sample_grid_gpts_per_s"] = round(pts / t_eval / 1e6, 2)
    L, ctx = res._L, res._h
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    ouv, suv = np.array([lo, lo], np.float32), np.array([step, step], np.float32)
    counts = (C.c_uint64 * 2)()
    call = lambda: L.rm_slice_contours(ctx, 1, fp(ouv), fp(suv), n, n, fp(heights), nl, 0.0, 0, counts, 2)  # noqa: E731
    assert call() == _ffi.RM_OK
    P, Cn = int(counts[0]), int(counts[1])
    points = np.empty((P, 3), np.float32)
    contours = np.empty((Cn, 4), np.uint32)
    layer_first = np.empty(nl + 1, np.uint32)

    def call_and_read():
        assert call() == _ffi.RM_OK
        assert L.rm_read_slices(ctx, points.ctypes.data, contours.ctypes.data, layer_first.ctypes.data, None, None, 0, None) == _ffi.RM_OK
    out["slice_contours_host_ms"] = host_ms(call, a.warmup, a.reps)
    out["slice_contours_and_read_host_ms"] = host_ms(call_and_read, a.warmup, a.reps)
    per_layer = np.bincount(contours[:, 2], weights=contours[:, 1], minlength=nl)
    out.update({"points_out": P, "contours": Cn, "closed": int(np.count_nonzero(contours[:, 3])),
                "longest_contour": int(contours[:, 1].max()) if Cn else 0, "fullest_layer_points": int(per_layer.max()),
                "ranking_rounds_per_pass": int(np.ceil(np.log2(max(per_layer.max(), 1)))),
                "batches": int(-(-pts // (1 << 27))) if n * n <= (1 << 27) else nl,
                "total_over_evaluation": round(out["slice_contours_host_ms"]["median"] / t_eval, 3)})
    res.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
