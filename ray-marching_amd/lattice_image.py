"""Pictures of class lattices for the command lines: what voxelize, thickness, supports and islands share for --image, --size
and --cut.  A lattice of class bytes (an occupancy, or an analysis' mask: 0 outside, 1 inside, 2.. what the analysis found) is
handed to RayMarchingResources.set_lattice without leaving the device, drawn by draw_lattice through camera.py's orbit camera
aimed at the lattice's box, and written as a PNG by orbit_batch's writer."""
import numpy as np

from . import _ffi, camera, orbit_batch

# The legend: the albedo of class 1 (inside), 2, 3, 4 of the masks; class 0 is empty and entry 0 is never looked up.
LEGEND = ((0.0, 0.0, 0.0), (0.72, 0.72, 0.75), (0.9, 0.15, 0.1), (0.1, 0.35, 0.9), (0.9, 0.75, 0.1))
LEGEND_NAMES = {"voxelize": ("", "inside"), "thickness": ("", "inside", "thin", "narrow"),
                "supports": ("", "inside", "overhang", "support on the plate", "support on the part"),
                "islands": ("", "inside", "island")}
AXES = {"x": 0, "y": 1, "z": 2}


def add_options(ap):
    ap.add_argument("--image", default=None, help="write a picture of the lattice here (.png)")
    ap.add_argument("--size", default="960x720", help="the picture's size, WxH")
    ap.add_argument("--cut", default=None, help="cut-away: show only the points lo <= index < hi of one axis, axis:lo:hi (e.g. z:0:40)")


def parse_size(text):
    """"960x720" -> (960, 720)."""
    parts = str(text).lower().split("x")
    if len(parts) != 2 or not all(p.strip().isdigit() for p in parts) or min(int(p) for p in parts) < 1:
        raise ValueError("--size: %r is not WxH" % (text,))
    return int(parts[0]), int(parts[1])


def parse_cut(text, shape):
    """"z:0:40" on a lattice of shape (nx, ny, nz) -> the window (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z); None -> None."""
    if text is None:
        return None
    parts = str(text).split(":")
    if len(parts) != 3 or parts[0].strip().lower() not in AXES or not all(p.strip().isdigit() for p in parts[1:]):
        raise ValueError("--cut: %r is not axis:lo:hi with axis x, y or z" % (text,))
    a, lo, hi = AXES[parts[0].strip().lower()], int(parts[1]), int(parts[2])
    if not lo < hi <= shape[a]:
        raise ValueError("--cut: [%d, %d) does not lie in the %d points of axis %s" % (lo, hi, shape[a], parts[0].strip()))
    window = [0, 0, 0] + [int(n) for n in shape]
    window[a], window[3 + a] = lo, hi
    return tuple(window)


def box_camera(origin, step, shape, yaw=-35.0, pitch=-25.0):
    """The orbit camera aimed at the centre of the lattice's box from 1.4 box diagonals away, on the side of shade_hit's light."""
    o, s = np.asarray(origin, dtype=np.float64), np.asarray(step, dtype=np.float64)
    lo, hi = o - 0.5 * s, o + (np.asarray(shape, dtype=np.float64) - 0.5) * s
    ctl = camera.OrbitCameraController.new([float(x) for x in 0.5 * (lo + hi)], 1.4 * float(np.linalg.norm(hi - lo)))
    ctl.update(camera.Orbit([float(yaw), float(pitch)]))
    return ctl.camera()


def device_bytes(res, shape, reader):
    """A new uint8 torch tensor (nz, ny, nx) on the context's GPU, filled by reader(address, stream) -- one of the
    read_*_device methods bound to its output -- on torch.cuda.current_stream()."""
    import torch
    dev = torch.device("cuda", res.device)
    out = torch.empty(tuple(shape)[::-1], dtype=torch.uint8, device=dev)
    reader(out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return out


def write(res, classes, origin, step, path, size="960x720", cut=None, palette=LEGEND):
    """set_lattice(classes), the legend palette through set_materials, one draw_lattice of the box camera, a PNG at `path`.
    Returns what a report says about the picture."""
    from . import renderer
    W, H = parse_size(size) if isinstance(size, str) else size
    lat = res.set_lattice(classes, origin, step)
    window = parse_cut(cut, lat.shape) if (cut is None or isinstance(cut, str)) else tuple(cut)
    res.set_materials([list(c) for c in palette])
    res.set_uniforms(renderer.prepare_uniforms((W, H), box_camera(lat.origin, lat.step, lat.shape)))
    res.set_output_format(_ffi.RM_FORMAT_RGBA8_UNORM)
    try:
        img = res.draw_lattice(W, H, window=window)
    finally:
        res.set_output_format(_ffi.RM_FORMAT_RGBA32F)
    with open(path, "wb") as f:
        f.write(orbit_batch.png_bytes(img))
    return {"file": path, "size": [W, H], "window": None if window is None else list(window), "points": lat.counts["points"],
            "bricks": lat.counts["bricks"]}
