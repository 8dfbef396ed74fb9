#!/usr/bin/env python3
"""rm_trace_rays against rm_cast_rays on the same rays (the pixel-centre rays of the still camera), device memory, alternating
in one process, timed with events on the stream.  Prints median / fastest / slowest of: the traversal march alone (counts and
spans only), the march writing its events, the whole call with the attribute pass (normals and ids), and the cast (ids only);
the sums of steps, and map_scene evaluations per second of the march and of the cast.  The attribute pass is the difference
of the two calls that write events.

  python tools/trace_probe.py --scene g32 --size 1920x1080 --t-max 20 --reps 15 --warmup 3"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ray_marching_amd import _ffi, camera, csg, renderer  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--t-max", type=float, default=20.0)
    ap.add_argument("--min-step", type=float, default=None)
    ap.add_argument("--max-steps", type=int, default=None, help="the traversal's step budget (default: rm_trace_defaults')")
    ap.add_argument("--max-events", type=int, default=8)
    ap.add_argument("--max-iter", type=int, default=256, help="the cast's step budget (limits.max_iter)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    W, H = (int(x) for x in a.size.lower().split("x"))
    n, K = W * H, a.max_events
    dev = torch.device("cuda", 0)
    res = renderer.RayMarchingResources(0)
    res.set_scene(csg.scene(a.scene))
    res.set_limits((0.01, 100.0, a.max_iter))
    ctl = camera.OrbitCameraController.new([0.0, 0.0, 0.0], 5.0)
    ctl.update(camera.Orbit([35.0, -25.0]))
    res.set_uniforms(renderer.prepare_uniforms((float(W), float(H)), ctl.camera()))
    rays = torch.empty((n, 6), dtype=torch.float32, device=dev)
    res.camera_rays(W, H, out=rays)
    p = renderer.trace_defaults()
    p[_ffi.RM_TRACE_T_MAX] = a.t_max
    if a.min_step is not None:
        p[_ffi.RM_TRACE_MIN_STEP] = a.min_step
    if a.max_steps is not None:
        p[_ffi.RM_TRACE_MAX_STEPS] = a.max_steps
    L = renderer.program_lipschitz(*res._program)
    p[_ffi.RM_TRACE_STEP_SCALE] = 1.0 / max(1.0, L)
    ev = torch.empty((n, K, 8), dtype=torch.float32, device=dev)
    eid = torch.empty((n, K, 4), dtype=torch.int32, device=dev)
    cnt = torch.empty((n, 4), dtype=torch.int32, device=dev)
    sp = torch.empty((n, 4), dtype=torch.float32, device=dev)
    ids = torch.empty((n, 4), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    both = _ffi.RM_MESH_NORMALS | _ffi.RM_MESH_IDS
    calls = {
        "trace: march, counts and spans only": lambda: res.trace_rays_device(n, rays.data_ptr(), p, K, 0, 0, 0, cnt.data_ptr(), sp.data_ptr(), stream=st),
        "trace: march writing events": lambda: res.trace_rays_device(n, rays.data_ptr(), p, K, 0, ev.data_ptr(), eid.data_ptr(), cnt.data_ptr(), sp.data_ptr(), stream=st),
        "trace: march + attributes (normals, ids)": lambda: res.trace_rays_device(n, rays.data_ptr(), p, K, both, ev.data_ptr(), eid.data_ptr(), cnt.data_ptr(), sp.data_ptr(), stream=st),
        "cast: ids only": lambda: res.cast_rays_device(n, rays.data_ptr(), 0, ids.data_ptr(), 0, stream=st),
    }
    times = {k: [] for k in calls}
    for r in range(a.warmup + a.reps):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    c4 = cnt.cpu().numpy().view("uint32")
    i4 = ids.cpu().numpy().view("uint32")
    trace_steps, stored, found = int(c4[:, 1].astype("uint64").sum()), int(c4[:, 3].astype("uint64").sum()), int(c4[:, 0].astype("uint64").sum())
    cast_steps, hits = int(i4[:, 1].astype("uint64").sum()), int((i4[:, 0] == _ffi.RM_HIT_SURFACE).sum())
    print("scene %s, %dx%d pixel-centre rays of the still camera (%d rays), traversal parameters %s (L = %g), K = %d;"
          % (a.scene, W, H, n, dict(zip(_ffi.TRACE_PARAM_NAMES, [float("%.6g" % v) for v in p])), L, K))
    print("cast limits (0.01, 100, %d); %d reps after %d warm-up rounds, alternating; times in ms from stream events" % (a.max_iter, a.reps, a.warmup))
    med = {}
    for name, t in times.items():
        med[name] = statistics.median(t)
        print("%-42s median %8.3f  fastest %8.3f  slowest %8.3f" % (name, med[name], min(t), max(t)))
    names = list(calls)
    attr = med[names[2]] - med[names[1]]
    print("attribute pass (scan, list, attributes): %.3f ms for %d stored events (%d found), %d evaluations (4 taps + 1 walk each)"
          % (attr, stored, found, 5 * stored))
    print("traversal: %d steps (%.2f per ray), out of steps %d rays, start inside %d rays" % (
        trace_steps, trace_steps / n, int(((c4[:, 2] & _ffi.RM_TRACE_OUT_OF_STEPS) != 0).sum()), int((c4[:, 2] & _ffi.RM_TRACE_START_INSIDE).sum())))
    print("cast:      %d steps (%.2f per ray), %d surface hits (one walk each)" % (cast_steps, cast_steps / n, hits))
    for name, evals in ((names[0], trace_steps), (names[1], trace_steps), (names[3], cast_steps + hits)):
        t = times[name]
        print("%-42s %.1f G evaluations/s at the median (%.1f .. %.1f over the repeats)" % (
            name, evals / med[name] / 1e6, evals / max(t) / 1e6, evals / min(t) / 1e6))
    # a wave marches until its last lane is done: the share of its lane-steps that evaluate something, and the rate per lane-step
    for label, steps, name in (("traversal", c4[:, 1], names[0]), ("cast", i4[:, 1], names[3])):
        s = np.zeros((n + 63) // 64 * 64, dtype=np.int64)
        s[:n] = steps
        per_wave = s.reshape(-1, 64)
        slots = int(per_wave.max(axis=1).sum()) * 64
        print("%-10s wave efficiency %.3f (steps / 64 x the longest ray of each wave of 64 consecutive rays); %.1f G lane-steps/s; "
              "steps per ray: median %d, 99th percentile %d, most %d"
              % (label, int(s.sum()) / slots, slots / med[name] / 1e6, int(np.median(steps)), int(np.percentile(steps, 99)), int(steps.max())))
    res.close()


if __name__ == "__main__":
    main()
