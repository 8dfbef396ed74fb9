#!/usr/bin/env python3
"""Lit rendering (rm_draw_lit) on one GPU against its two yardsticks, 1920x1080, still camera, limits
0.01 / 100 / 256, scenes g32 (chain loop) and mat_mix (general loop).

  --count   no GPU: the map_scene evaluations of the identity and the default configuration from tests/light_ref.py, over a
            seeded sample of 2 x 2 pixel blocks (one block = one wave of the kernel) scaled up to the frame, per phase; and,
            per phase, the evaluations a wave spends -- the largest count among its 64 lanes -- next to the sum over its
            lanes: lanes / (64 x wave) is the share of lanes that are busy.  Writes a JSON file (--counts).
  default   on the GPU, alternating within one process, per repetition: (a) the sixteen rm_cast_rays launches (colour only)
            over the sample rays rm_camera_rays made beforehand, (b) the identity lit draw, (c) the default lit draw, (d) rm_draw.
            Device events around each leg on one stream; median, minimum and maximum over --reps after --warmup rounds.
            Prints one JSON line; evaluation rates use the counts file.

usage: tools/lit_probe.py --count; tools/lit_probe.py [--reps N] > profiles/r06_lit_probe.txt"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

W, H = 1920, 1080
LIMITS = (0.01, 100.0, 256)
SCENES = ("g32", "mat_mix")
MATERIALS = [(0.4, 0.7, 0.1), (0.9, 0.15, 0.1), (0.1, 0.3, 0.9), (0.95, 0.9, 0.2), (0.8, 0.8, 0.8), (0.6, 0.1, 0.7)]
COUNTS = os.path.join(ROOT, "profiles", "r06_lit_eval_counts.json")


def still_camera():
    from ray_marching_amd import camera, renderer
    ctl = camera.OrbitCameraController.new([0.0, 0.0, 0.0], 5.0)
    ctl.update(camera.Orbit([35.0, -25.0]))
    return renderer.prepare_uniforms((W, H), ctl.camera())


def count(blocks, path):
    import light_ref
    from ray_marching_amd import csg
    u = still_camera()
    ud = {"viewport_extent": list(u.viewport_extent), "inv_proj": list(u.inv_proj), "inv_view": list(u.inv_view)}
    rng = np.random.default_rng(13)
    at = rng.choice((W // 2) * (H // 2), blocks, replace=False)
    bx, by = at % (W // 2), at // (W // 2)
    px = (2 * bx[:, None] + np.array([0, 1, 0, 1])).ravel()      # the four pixels of each block, in lane order
    py = (2 * by[:, None] + np.array([0, 0, 1, 1])).ravel()
    scale = (W // 2) * (H // 2) / blocks
    out = {"frame": [W, H], "limits": list(LIMITS), "sampled_blocks": blocks, "sampled_pixels": 4 * blocks,
           "note": "seeded sample of 2x2 blocks, scaled by %.1f to the frame" % scale}
    for scene in SCENES:
        cc, words = csg.serialize(csg.scene(scene))
        table = MATERIALS if scene == "mat_mix" else None
        for cfg, light in (("identity", light_ref.params(**light_ref.IDENTITY)), ("default", light_ref.params())):
            _, evals, parts = light_ref.render_pixels(px, py, ud, LIMITS, cc, words, W, H, materials=table, light=light, detail=True)
            e = {"evaluations": int(round(float(evals.sum()) * scale))}
            lanes_all = wave_all = 0
            for k in light_ref.PHASES:
                lanes = parts[k].reshape(blocks, 64)             # one wave per row
                wave = lanes.max(axis=1)
                e[k] = {"lane_evaluations": int(round(float(lanes.sum()) * scale)), "wave_evaluations": int(round(float(wave.sum()) * scale)),
                        "busy_lanes": round(float(lanes.sum()) / max(64.0 * float(wave.sum()), 1.0), 4),
                        "lanes_taking_part": round(float((lanes > 0).mean()), 4)}
                lanes_all += float(lanes.sum())
                wave_all += float(wave.sum())
            e["wave_evaluations"] = int(round(wave_all * scale))
            e["busy_lanes"] = round(lanes_all / (64.0 * wave_all), 4)
            out["%s_%s" % (scene, cfg)] = e
            print(scene, cfg, json.dumps(e), file=sys.stderr, flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def measure(a):
    import torch
    from ray_marching_amd import _ffi, csg, renderer
    import light_ref
    dev = torch.device("cuda", 0)
    counts = json.load(open(a.counts)) if os.path.exists(a.counts) else {}
    res = renderer.RayMarchingResources(0)
    res.set_materials(MATERIALS)
    res.set_limits(renderer.RayMarchLimits(*LIMITS))
    res.set_uniforms(still_camera())
    res.set_option(_ffi.RM_OPT_SPECIALIZE, 2)
    n = W * H
    rays = [torch.empty((n, 6), dtype=torch.float32, device=dev) for _ in range(16)]
    for s in range(16):
        res.camera_rays(W, H, sample=s, out=rays[s])
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    img = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    ident = dict(zip(light_ref.NAMES, [float(v) for v in light_ref.params(**light_ref.IDENTITY)]))
    deflt = dict(zip(light_ref.NAMES, [float(v) for v in light_ref.params()]))

    def cast16():
        for s in range(16):
            res.cast_rays_device(n, rays[s].data_ptr(), rgb_ptr=rgb.data_ptr(), stream=st)

    def lit(cfg):
        res.set_lighting(**cfg)
        res.draw_lit_device(W, H, img.data_ptr(), stream=st)

    legs = (("cast16", cast16), ("lit_identity", lambda: lit(ident)), ("lit_default", lambda: lit(deflt)),
            ("draw", lambda: res.draw_device(W, H, img.data_ptr(), stream=st)))
    out = {"gpu": torch.cuda.get_device_name(dev), "frame": [W, H], "limits": list(LIMITS), "reps": a.reps, "warmup": a.warmup}
    for scene in SCENES:
        res.set_scene(csg.scene(scene))
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
        r["lit_identity_over_cast16"] = round(r["lit_identity"]["median_ms"] / r["cast16"]["median_ms"], 4)
        r["lit_default_over_identity"] = round(r["lit_default"]["median_ms"] / r["lit_identity"]["median_ms"], 4)
        for cfg in ("identity", "default"):
            c = counts.get("%s_%s" % (scene, cfg))
            if c:
                ms = r["lit_" + cfg]["median_ms"]
                r["lit_%s_g_lane_evals_per_s" % cfg] = round(c["evaluations"] / ms / 1e6, 2)
                r["lit_%s_g_wave_evals_x64_per_s" % cfg] = round(64.0 * c["wave_evaluations"] / ms / 1e6, 2)
                r["lit_%s_busy_lanes" % cfg] = c["busy_lanes"]
        out[scene] = r
    res.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--blocks", type=int, default=5000, help="--count: 2 x 2 blocks sampled (5000 = 20 000 pixels)")
    ap.add_argument("--counts", default=COUNTS)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.count:
        count(a.blocks, a.counts)
    else:
        measure(a)


if __name__ == "__main__":
    main()
