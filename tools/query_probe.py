#!/usr/bin/env python3
"""Scene-query throughput on one GPU (rm_query_points, rm_cast_rays, pick); prints one JSON line.

  points: 2^24 seeded points uniform in [-8, 8]^3, scenes g32 and mat_mix, distance only and with normal + ids
  rays:   the 2 073 600 centre rays of the 1920x1080 metric camera (g32, limits 0.01 / 100 / 256)
  pick:   median host-to-host latency of 100 warm RayMarchingResources.pick calls

Kernel times are device events around each call on the caller's stream (median over --reps after --warmup calls); the
device buffers are torch tensors.  usage: tools/query_probe.py [--reps N] > profiles/r04_scene_queries.txt"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ray_marching_amd import _ffi, camera, csg, renderer  # noqa: E402

MATERIALS = [(0.4, 0.7, 0.1), (0.9, 0.15, 0.1), (0.1, 0.3, 0.9), (0.95, 0.9, 0.2), (0.8, 0.8, 0.8), (0.6, 0.1, 0.7)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream  # noqa: E731
    res = renderer.RayMarchingResources(0)
    res.set_materials(MATERIALS)
    res.set_limits(renderer.RayMarchLimits(0.01, 100.0, 256))
    n = 1 << 24
    rng = np.random.default_rng(2024)
    pts = torch.from_numpy(rng.uniform(-8.0, 8.0, (n, 3)).astype(np.float32)).to(dev)
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
    ids = torch.empty((n, 2), dtype=torch.int32, device=dev)
    out = {"points": n, "gpu": torch.cuda.get_device_name(dev)}
    for scene in ("g32", "mat_mix"):
        res.set_scene(csg.scene(scene))
        t_d = timed(torch, lambda: res.query_points_device(n, pts.data_ptr(), dist.data_ptr(), stream=stream()), a.warmup, a.reps)
        t_f = timed(torch, lambda: res.query_points_device(n, pts.data_ptr(), dist.data_ptr(), nrm.data_ptr(), ids.data_ptr(),
                                                           stream=stream()), a.warmup, a.reps)
        out["points_%s_dist_ms" % scene] = round(t_d, 4)
        out["points_%s_dist_gpts_per_s" % scene] = round(n / t_d / 1e6, 2)
        out["points_%s_full_ms" % scene] = round(t_f, 4)
        out["points_%s_full_over_dist" % scene] = round(t_f / t_d, 2)
    del pts, dist, nrm, ids
    # centre rays of the metric frame
    W, H = 1920, 1080
    res.set_scene(csg.scene("g32"))
    ctl = camera.OrbitCameraController.new([0.0, 0.0, 0.0], 5.0)
    ctl.update(camera.Orbit([35.0, -25.0]))
    res.set_uniforms(renderer.prepare_uniforms((W, H), ctl.camera()))
    nr = W * H
    rays = torch.empty((nr, 6), dtype=torch.float32, device=dev)
    res.camera_rays(W, H, out=rays)
    hit = torch.empty((nr, 8), dtype=torch.float32, device=dev)
    rids = torch.empty((nr, 4), dtype=torch.int32, device=dev)
    rgb = torch.empty((nr, 3), dtype=torch.float32, device=dev)
    t_r = timed(torch, lambda: res.cast_rays_device(nr, rays.data_ptr(), hit.data_ptr(), rids.data_ptr(), rgb.data_ptr(),
                                                    stream=stream()), a.warmup, a.reps)
    # map_scene evaluations of these rays: the march loop's (the steps rm_cast_rays reports; tests/test_gpu_query.py checks them
    # against the oracle's march_steps counter), plus 4 taps and 1 leaf walk per surface hit
    r = rids.cpu().numpy().view(np.uint32)
    steps, hits = int(r[:, 1].astype(np.uint64).sum()), int((r[:, 0] == _ffi.RM_HIT_SURFACE).sum())
    evals = steps + 5 * hits
    out.update({"rays": nr, "rays_ms": round(t_r, 4), "rays_march_steps": steps, "rays_surface_hits": hits,
                "rays_evaluations": evals, "rays_g_evals_per_s": round(evals / t_r / 1e6, 2),
                "rays_eval_rate_over_points_g32_dist": round((evals / t_r) / (n / out["points_g32_dist_ms"]), 3)})
    # pick: host to host, warm context
    for _ in range(10):
        res.pick(W, H, W // 2, H // 2)
    lat = []
    for _ in range(100):
        t0 = time.perf_counter()
        res.pick(W, H, W // 2, H // 2)
        lat.append((time.perf_counter() - t0) * 1e3)
    out["pick_median_ms"] = round(float(np.median(lat)), 4)
    out["pick_p90_ms"] = round(float(np.percentile(lat, 90)), 4)
    res.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
