"""Thickness images and wall thickness from RayMarchingResources.trace_rays: how much material a ray
passes through, and how far behind a surface point the part ends.

  python -m ray_marching_amd.xray --scene g32 --size 640x360 --t-max 20 out      (writes out.npy and out.png)
  python -m ray_marching_amd.xray --scene g32 --walls --lo -2.5 --hi 2.5 --res 128

thickness_image gives, per pixel, the length inside the solid along the ray through the pixel centre (float32 .npy, and a
16-bit greyscale PNG scaled to the largest value).  wall_thickness casts one ray per mesh vertex from the vertex along
-normal, starting just inside, and reports the t of the first EXIT.  Both take any object with camera_rays / trace_rays
(RayMarchingResources, or a stand-in), and numpy arrays from it."""
import argparse
import struct
import sys
import zlib

import numpy as np

from ._ffi import RM_TRACE_EXIT
from .orbit_batch import PNG_IEND, PNG_SIGNATURE, png_chunk


def thickness_image(renderer, W, H, **trace):
    """(H, W) float32: `length` of trace_rays along the pixel-centre rays of camera_rays(W, H); trace: its keyword
    parameters (t_min, t_max, min_step, step_scale, level, max_steps).  No event is stored beyond the one slot the call needs."""
    rays = renderer.camera_rays(W, H)
    out = renderer.trace_rays(rays, max_events=1, normals=False, ids=False, **trace)
    return np.asarray(out["length"], dtype=np.float32).reshape(H, W)


def png16_bytes(img, scale=None, level=6):
    """16-bit greyscale PNG (colour type 0, no interlace, filter 0 on every row) of a 2-D array: value * 65535 / scale,
    clipped; scale None: the largest finite value (an image of zeros stays zeros).  Standard library only."""
    a = np.asarray(img, dtype=np.float64)
    H, W = a.shape
    if scale is None:
        finite = a[np.isfinite(a)]
        scale = float(finite.max()) if finite.size and finite.max() > 0 else 1.0
    v = np.clip(np.rint(np.nan_to_num(a, nan=0.0, posinf=scale, neginf=0.0) * (65535.0 / scale)), 0, 65535).astype(">u2")
    rows = np.zeros((H, 1 + 2 * W), dtype=np.uint8)
    rows[:, 1:] = v.view(np.uint8).reshape(H, 2 * W)
    ihdr = struct.pack(">IIBBBBB", W, H, 16, 0, 0, 0, 0)
    return PNG_SIGNATURE + png_chunk(b"IHDR", ihdr) + png_chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + PNG_IEND


def write_thickness(img, stem):
    """stem.npy (the float32 values) and stem.png (16-bit, scaled to the largest value); returns the two paths."""
    np.save(stem + ".npy", np.asarray(img, dtype=np.float32))
    with open(stem + ".png", "wb") as f:
        f.write(png16_bytes(img))
    return stem + ".npy", stem + ".png"


def wall_thickness(renderer, mesh, start=None, max_events=4, **trace):
    """Per vertex of `mesh` (vertices and normals, as extract_mesh returns them): the t of the first EXIT along -normal,
    from t_min = `start` on (default: 4 * min_step, just inside the surface the vertex lies on); +inf where the ray finds
    no exit within t_max (or within the first max_events events), NaN where the vertex has no normal.  Returns (thickness
    (V,) float32, the dict of trace_rays)."""
    v = np.asarray(mesh.vertices, dtype=np.float32)
    n = np.asarray(mesh.normals, dtype=np.float32)
    if start is None:
        min_step = trace.get("min_step")
        if min_step is None:
            min_step = renderer.trace_defaults()["min_step"]
        start = 4.0 * float(min_step)
    trace = dict(trace, t_min=start)
    out = renderer.trace_rays(np.ascontiguousarray(np.concatenate([v, -n], axis=1)), max_events=max_events, normals=False, ids=False,
                              **trace)
    kind, t = np.asarray(out["kind"]), np.asarray(out["t"], dtype=np.float32)
    is_exit = kind == RM_TRACE_EXIT
    first = np.argmax(is_exit, axis=1)
    thick = np.where(is_exit.any(axis=1), t[np.arange(len(t)), first], np.float32(np.inf)).astype(np.float32)
    thick[~np.isfinite(n).all(axis=1)] = np.nan
    return thick, out


def summary(thick, percentiles=(1, 5, 25, 50, 75, 95, 99)):
    """Minimum, percentiles and the count without an exit, over the vertices that have one, as a dict."""
    t = np.asarray(thick, dtype=np.float64)
    ok = t[np.isfinite(t)]
    out = {"vertices": int(t.size), "no_exit": int(np.isinf(t).sum()), "no_normal": int(np.isnan(t).sum())}
    if ok.size:
        out["min"] = float(ok.min())
        out.update({"p%d" % p: float(np.percentile(ok, p)) for p in percentiles})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ray_marching_amd.xray", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32", help="a csg.scene name (g1, g8, g32, g32_balanced, mat_mix, ...)")
    ap.add_argument("--size", default="640x360", help="WxH of the thickness image")
    ap.add_argument("--yaw", type=float, default=35.0)
    ap.add_argument("--pitch", type=float, default=-25.0)
    ap.add_argument("--radius", type=float, default=5.0)
    ap.add_argument("--t-max", type=float, default=20.0)
    ap.add_argument("--min-step", type=float, default=None)
    ap.add_argument("--level", type=float, default=None)
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--walls", action="store_true", help="wall thickness at the vertices of the extracted mesh instead of an image")
    ap.add_argument("--lo", type=float, default=-2.5)
    ap.add_argument("--hi", type=float, default=2.5)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("out", nargs="?", default="thickness", help="output stem: <out>.npy and <out>.png (or <out>.npy with --walls)")
    a = ap.parse_args(argv)
    from . import camera, csg, renderer
    res = renderer.RayMarchingResources(a.device)
    trace = dict(t_max=a.t_max, min_step=a.min_step, level=a.level, max_steps=a.max_steps)
    try:
        res.set_scene(csg.scene(a.scene))
        if a.walls:
            mesh = res.extract_mesh([a.lo] * 3, [a.hi] * 3, [a.res] * 3, level=0.0 if a.level is None else a.level, normals=True, ids=False)
            thick, _ = wall_thickness(res, mesh, **trace)
            np.save(a.out + ".npy", thick)
            print("%s.npy: wall thickness at %d vertices: %s" % (a.out, len(thick), summary(thick)))
        else:
            W, H = (int(x) for x in a.size.lower().split("x"))
            ctl = camera.OrbitCameraController.new([0.0, 0.0, 0.0], a.radius)
            ctl.update(camera.Orbit([a.yaw, a.pitch]))
            res.set_uniforms(renderer.prepare_uniforms((float(W), float(H)), ctl.camera()))
            img = thickness_image(res, W, H, **trace)
            paths = write_thickness(img, a.out)
            print("%s, %s: %dx%d, thickness up to %.6g, %d pixels see the solid" % (paths + (W, H, float(img.max()), int((img > 0).sum()))))
    finally:
        res.close()


if __name__ == "__main__":
    sys.exit(main())
