#!/usr/bin/env python3
"""The G-buffer draw (rm_draw_gbuffer) on one GPU against its yardsticks, 1920x1080, still camera,
limits 0.01 / 100 / 256, scenes g32 (chain loop) and mat_mix (general loop with the leaf walk).

Legs, alternating within one process, per repetition:
  cast16          yardstick A: sixteen rm_camera_rays + rm_cast_rays(out_hit, out_ids) pairs on device arrays (what a user
                  does without the G-buffer draw; the host-side reduction of the 16 records per pixel is left out)
  gbuffer_all     rm_draw_gbuffer(RM_SAMPLE_ALL) with all three outputs and a selection (the first half of the commands)
  lit_identity    yardstick B: rm_draw_lit with S = 0 and A = 0 (the same march and taps, a walk for tagged programs only,
                  16 B per pixel)
  cast1           one rm_camera_rays(RM_SAMPLE_CENTER) + rm_cast_rays(out_hit, out_ids) pair
  gbuffer_center  rm_draw_gbuffer(RM_SAMPLE_CENTER) with all three outputs
Device events around each leg on one stream; median, minimum and maximum over --reps after --warmup rounds.  The map_scene
evaluations of a frame are exact, from the G-buffer itself: the step sum (march), 4 per surface sample (taps), 1 per surface
sample (walk).  Prints one JSON line.

usage: tools/gbuffer_probe.py [--reps N] > profiles/r07_gbuffer_probe.txt"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

W, H = 1920, 1080
LIMITS = (0.01, 100.0, 256)
SCENES = ("g32", "mat_mix")
MATERIALS = [(0.4, 0.7, 0.1), (0.9, 0.15, 0.1), (0.1, 0.3, 0.9), (0.95, 0.9, 0.2), (0.8, 0.8, 0.8), (0.6, 0.1, 0.7)]


def still_camera():
    from ray_marching_amd import camera, renderer
    ctl = camera.OrbitCameraController.new([0.0, 0.0, 0.0], 5.0)
    ctl.update(camera.Orbit([35.0, -25.0]))
    return renderer.prepare_uniforms((W, H), ctl.camera())


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def spread(s):
    return s["max_ms"] - s["min_ms"]


def popcount(a):
    a = a.astype(np.uint32)
    return sum(int(((a >> np.uint32(b)) & np.uint32(1)).sum()) for b in range(17))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from ray_marching_amd import _ffi, csg, renderer
    dev = torch.device("cuda", 0)
    res = renderer.RayMarchingResources(0)
    res.set_materials(MATERIALS)
    res.set_limits(renderer.RayMarchLimits(*LIMITS))
    res.set_uniforms(still_camera())
    res.set_lighting(shadow=0.0, ao=0.0)
    n = W * H
    rays = torch.empty((n, 6), dtype=torch.float32, device=dev)
    hit = torch.empty((n, 8), dtype=torch.float32, device=dev)
    ids = torch.empty((n, 4), dtype=torch.int32, device=dev)
    masks = torch.empty((n, 4), dtype=torch.int32, device=dev)
    img = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def pair(sample):
        res.camera_rays_device(W, H, 0, 0, W, H, rays.data_ptr(), sample=sample, stream=st)
        res.cast_rays_device(n, rays.data_ptr(), hit_ptr=hit.data_ptr(), ids_ptr=ids.data_ptr(), stream=st)

    def cast16():
        for s in range(16):
            pair(s)

    out = {"gpu": torch.cuda.get_device_name(dev), "frame": [W, H], "limits": list(LIMITS), "reps": a.reps, "warmup": a.warmup}
    for scene in SCENES:
        res.set_scene(csg.scene(scene))
        cc, _ = csg.serialize(csg.scene(scene))
        sel = (0, cc // 2)

        def gbuffer(sample):
            res.draw_gbuffer_device(W, H, hit.data_ptr(), ids.data_ptr(), masks.data_ptr(), sample=sample, select=sel, stream=st)

        legs = (("cast16", cast16), ("gbuffer_all", lambda: gbuffer(_ffi.RM_SAMPLE_ALL)),
                ("lit_identity", lambda: res.draw_lit_device(W, H, img.data_ptr(), stream=st)),
                ("cast1", lambda: pair(_ffi.RM_SAMPLE_CENTER)), ("gbuffer_center", lambda: gbuffer(_ffi.RM_SAMPLE_CENTER)))
        times = {k: [] for k, _ in legs}
        for rep in range(a.warmup + a.reps):
            for k, fn in legs:                                   # the legs alternate within every round
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    times[k].append(e0.elapsed_time(e1))
        r = {k: stats(v) for k, v in times.items()}
        r["gbuffer_all_over_cast16"] = round(r["gbuffer_all"]["median_ms"] / r["cast16"]["median_ms"], 4)
        r["cast16_minus_gbuffer_all_ms"] = round(r["cast16"]["median_ms"] - r["gbuffer_all"]["median_ms"], 4)
        r["larger_spread_all_ms"] = round(max(spread(r["cast16"]), spread(r["gbuffer_all"])), 4)
        r["gbuffer_all_over_lit_identity"] = round(r["gbuffer_all"]["median_ms"] / r["lit_identity"]["median_ms"], 4)
        r["gbuffer_center_over_cast1"] = round(r["gbuffer_center"]["median_ms"] / r["cast1"]["median_ms"], 4)
        r["gbuffer_center_minus_cast1_ms"] = round(r["gbuffer_center"]["median_ms"] - r["cast1"]["median_ms"], 4)
        r["larger_spread_center_ms"] = round(max(spread(r["cast1"]), spread(r["gbuffer_center"])), 4)
        # evaluations and bytes of the two G-buffer frames, from their own output
        for form, sample in (("all", _ffi.RM_SAMPLE_ALL), ("center", _ffi.RM_SAMPLE_CENTER)):
            g = res.draw_gbuffer(W, H, sample=sample, select=sel)
            march = int(g["steps"].astype(np.uint64).sum())
            surface = popcount(g["surface_mask"])
            evals = {"march": march, "taps": 4 * surface, "walk": surface, "surface_samples": surface,
                     "selected_samples": popcount(g["selected_mask"])}
            ms = r["gbuffer_" + form]["median_ms"]
            r["gbuffer_%s_evaluations" % form] = evals
            r["gbuffer_%s_g_evals_per_s" % form] = round((march + 5 * surface) / ms / 1e6, 2)
            r["gbuffer_%s_write_gb_per_s" % form] = round(n * 64 / ms / 1e6, 2)
        out[scene] = r
    res.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
