"""Offline camera-orbit batch (BASELINE config 5): N frames of one scene, frame f at
yaw = 2*pi*f/N, sharded over the ranks of one node (frame f -> rank f % world, no collective), written as binary PPM or PNG.

  output stage   frames are rendered in an 8-bit format (4 B/pixel on the device and over PCIe, a quarter of RGBA32F);
                 the RGBA32F path stays available (--format f32 writes raw little-endian float32 RGBA, .rgba32f)
  async drain    a ring of device buffers and pinned host buffers per rank: frame i+1 renders while frame i is copied
                 to the host on a second stream and writer threads turn the previous ones into files
  resume         a frame whose file already exists with the exact expected size is skipped; files are written to a
                 temporary name and renamed, so an interrupted run never leaves a plausible-looking partial frame

The reference has no offline mode (it only draws into an eframe window, main.rs:14-19); this is the batch driver
the north-star configuration asks for, built on the same rm_draw entry point the window path uses.

  python -m ray_marching_amd.orbit_batch --out-dir /tmp/orbit --frames 1024 --width 3840 --height 2160
  python -m ray_marching_amd.orbit_batch --out-dir /tmp/orbit_lit --lit --shadow 1 --ao 1 --light 2 -5 3 ...    (soft shadows and
                 ambient occlusion through rm_draw_lit; orbit.json records the lighting, an unlit job's manifest is unchanged)
  python -m torch.distributed.run --nproc-per-node 8 ... -m ray_marching_amd.orbit_batch ...    (one rank per GPU)
"""
import argparse
import json
import math
import os
import queue
import struct
import threading
import time
import zlib

import numpy as np

from . import shard


EXT = {"ppm": "ppm", "png": "png", "f32": "rgba32f"}
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
PNG_IEND = struct.pack(">I", 0) + b"IEND" + struct.pack(">I", zlib.crc32(b"IEND"))


def frame_path(out_dir, f, fmt):
    return os.path.join(out_dir, "frame_%05d.%s" % (f, EXT[fmt]))


def ppm_header(W, H):
    return b"P6\n%d %d\n255\n" % (W, H)


def expected_size(W, H, fmt):
    """Exact file size of a finished frame; None for PNG (compressed: see png_is_complete)."""
    if fmt == "png":
        return None
    return len(ppm_header(W, H)) + W * H * 3 if fmt != "f32" else W * H * 16


def png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def png_bytes(img, level=1):
    """8-bit RGB PNG (colour type 2, no interlace, filter 0 on every row) of an (H, W, >=3) uint8 array, standard library
    only.  level 1: the batch is bound by the file system, not by the size of the files."""
    H, W = img.shape[:2]
    rows = np.empty((H, 1 + 3 * W), dtype=np.uint8)
    rows[:, 0] = 0
    rows[:, 1:] = np.ascontiguousarray(img[..., :3]).reshape(H, 3 * W)
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
    return PNG_SIGNATURE + png_chunk(b"IHDR", ihdr) + png_chunk(b"IDAT", zlib.compress(memoryview(rows).cast("B"), level)) + PNG_IEND


def png_is_complete(path, W, H):
    """A finished PNG of the expected size: signature, an IHDR with these dimensions, the IEND trailer at the very end
    (files are renamed into place only when complete, so this is a consistency check, not a parse)."""
    try:
        with open(path, "rb") as fh:
            head = fh.read(33)
            fh.seek(-12, os.SEEK_END)
            tail = fh.read(12)
    except OSError:
        return False
    return (len(head) == 33 and head[:8] == PNG_SIGNATURE and head[12:16] == b"IHDR"
            and struct.unpack(">II", head[16:24]) == (W, H) and tail == PNG_IEND)


def frame_is_done(out_dir, f, W, H, fmt):
    p = frame_path(out_dir, f, fmt)
    if fmt == "png":
        return png_is_complete(p, W, H)
    try:
        return os.path.getsize(p) == expected_size(W, H, fmt)
    except OSError:
        return False


def frames_todo(out_dir, n_frames, rank, world, W, H, fmt):
    """This rank's frames that still have to be rendered (resume by frame index)."""
    return [f for f in shard.frames_of_rank(n_frames, rank, world) if not frame_is_done(out_dir, f, W, H, fmt)]


def write_frame(out_dir, f, img, fmt):
    """img: (H, W, 3) or (H, W, 4) uint8 in RGB(A) order, or float32 RGBA for fmt == 'f32'.  Atomic: temp file + rename."""
    p = frame_path(out_dir, f, fmt)
    tmp = p + ".part"
    with open(tmp, "wb") as fh:
        if fmt == "f32":
            fh.write(memoryview(np.ascontiguousarray(img, dtype=np.float32)).cast("B"))
        elif fmt == "png":
            fh.write(png_bytes(img))
        else:
            H, W = img.shape[:2]
            fh.write(ppm_header(W, H))
            fh.write(memoryview(np.ascontiguousarray(img[..., :3])).cast("B"))   # no copy when the image is already RGB
    os.replace(tmp, p)
    return p


def check_manifest(args):
    """Resume is by frame index and file size only, so the directory must belong to the same job: the first run writes
    orbit.json, later runs refuse to mix parameters (a different frame count changes every camera)."""
    want = {"frames": args.frames, "width": args.width, "height": args.height, "scene": args.scene,
            "max_iter": args.max_iter, "format": args.format}
    want.update(lighting_of(args) or {})      # lighting keys only for a lit job: an unlit directory resumes as before
    path = os.path.join(args.out_dir, "orbit.json")
    try:
        with open(path) as fh:
            have = json.load(fh)
    except (OSError, ValueError):
        have = None
    if have is None:
        tmp = path + ".part%d" % os.getpid()
        with open(tmp, "w") as fh:
            json.dump(want, fh)
        os.replace(tmp, path)
    elif have != want:
        raise SystemExit("%s was written with %s; this run asks for %s" % (args.out_dir, have, want))


def lighting_of(args):
    """The manifest's lighting keys of a --lit job, None for an unlit one (whose manifest and frames stay as they were)."""
    if not getattr(args, "lit", False):
        return None
    return {"lit": True, "shadow": float(args.shadow), "ao": float(args.ao), "light": [float(v) for v in args.light]}


def orbit_yaw(f, n_frames):
    return 2.0 * math.pi * f / n_frames


def render_batch(args, rank=0, world=1, device=0, log=None):
    """Renders this rank's missing frames.  Returns a summary dict."""
    import torch
    from . import _ffi, camera, csg, renderer

    W, H = args.width, args.height
    os.makedirs(args.out_dir, exist_ok=True)
    check_manifest(args)
    todo = frames_todo(args.out_dir, args.frames, rank, world, W, H, args.format)
    mine = len(shard.frames_of_rank(args.frames, rank, world))
    summary = {"rank": rank, "frames_assigned": mine, "frames_skipped": mine - len(todo), "frames_rendered": 0,
               "seconds": 0.0}
    if not todo:
        return summary
    torch.cuda.set_device(device)
    res = renderer.RayMarchingResources(device)
    res.set_option(_ffi.RM_OPT_SPECIALIZE, 2)       # static scene: compile its kernel once, before the first frame
    res.set_limits(renderer.RayMarchLimits(0.01, 100.0, args.max_iter))
    node = csg.scene(args.scene)
    cc, words = csg.serialize(node)
    if len(words) > 255:
        res.resize_command_buffer(4 * (len(words) + 1 + 63) // 64 * 64)
    res.set_program(cc, words)
    lit = lighting_of(args)
    if lit:
        res.set_lighting(pos=lit["light"], shadow=lit["shadow"], ao=lit["ao"])
    draw = res.draw_lit_device if lit else res.draw_device
    f32 = args.format == "f32"
    res.set_output_format(_ffi.RM_FORMAT_RGBA32F if f32 else _ffi.RM_FORMAT_RGBA8_UNORM)
    dt = torch.float32 if f32 else torch.uint8
    n_slots, n_writers = max(2, args.slots), max(1, args.writers)
    dev = [torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(n_slots)]
    # PPM holds RGB: the alpha plane is dropped on the device (a strided copy on the drain stream), so 3 B/px cross
    # PCIe and the writer threads hand the pinned buffer to the file as it is
    drain = dev if f32 else [torch.empty((H, W, 3), dtype=dt, device="cuda") for _ in range(n_slots)]
    host = [torch.empty((H, W, 4 if f32 else 3), dtype=dt).pin_memory() for _ in range(n_slots)]
    render_s, copy_s = torch.cuda.Stream(), torch.cuda.Stream()
    rendered = [torch.cuda.Event() for _ in range(n_slots)]
    copied = [torch.cuda.Event() for _ in range(n_slots)]
    free = [threading.Semaphore(1) for _ in range(n_slots)]       # host[slot] may be overwritten
    jobs = queue.Queue()
    errors = []

    def writer():
        while True:
            job = jobs.get()
            if job is None:
                return
            f, slot = job
            try:
                copied[slot].synchronize()
                write_frame(args.out_dir, f, host[slot].numpy(), args.format)
            except Exception as e:      # surfaced by the main thread
                errors.append(e)
            finally:
                free[slot].release()

    threads = [threading.Thread(target=writer, daemon=True) for _ in range(n_writers)]
    for th in threads:
        th.start()
    ctl = camera.OrbitCameraController.new([0.0, 0.0, 0.0], 5.0)
    t0 = time.perf_counter()
    for i, f in enumerate(todo):
        slot = i % n_slots
        free[slot].acquire()            # the writer is done with host[slot] (and so is the copy into it)
        if errors:
            break
        ctl.set_angles(orbit_yaw(f, args.frames), -0.25, 5.0)
        res.set_uniforms(renderer.prepare_uniforms((float(W), float(H)), ctl.camera()))
        render_s.wait_event(copied[slot])          # dev[slot] was read by the copy n_slots frames ago
        draw(W, H, dev[slot].data_ptr(), stream=render_s.cuda_stream)
        rendered[slot].record(render_s)
        copy_s.wait_event(rendered[slot])
        with torch.cuda.stream(copy_s):
            if not f32:
                drain[slot].copy_(dev[slot][..., :3])
            host[slot].copy_(drain[slot], non_blocking=True)
        copied[slot].record(copy_s)
        jobs.put((f, slot))
        summary["frames_rendered"] += 1
        if log and (i + 1) % 64 == 0:
            log("rank %d: %d / %d frames" % (rank, i + 1, len(todo)))
    for _ in threads:
        jobs.put(None)
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    summary["seconds"] = time.perf_counter() - t0
    res.close()
    if errors:
        raise errors[0]
    return summary


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--out-dir", required=True)
    p.add_argument("--frames", type=int, default=1024)
    p.add_argument("--width", type=int, default=3840)
    p.add_argument("--height", type=int, default=2160)
    p.add_argument("--scene", default="g32")
    p.add_argument("--max-iter", type=int, default=256)
    p.add_argument("--format", choices=["ppm", "png", "f32"], default="ppm",
                   help="ppm / png: 8-bit output stage (png: zlib level 1, standard library only); f32: raw RGBA32F")
    p.add_argument("--slots", type=int, default=4, help="device / pinned-host buffer pairs in flight")
    p.add_argument("--writers", type=int, default=3, help="file-writer threads")
    p.add_argument("--lit", action="store_true", help="soft shadows and ambient occlusion (rm_draw_lit; DESIGN.md section 13)")
    p.add_argument("--shadow", type=float, default=1.0, metavar="S", help="with --lit: strength of the shadow term, 0..1")
    p.add_argument("--ao", type=float, default=1.0, metavar="A", help="with --lit: strength of the occlusion term, 0..1")
    p.add_argument("--light", type=float, nargs=3, default=[2.0, -5.0, 3.0], metavar=("X", "Y", "Z"),
                   help="with --lit: the light's position parameter (the reference's: 2 -5 3)")
    p.add_argument("--all-ranks-on-device0", action="store_true", help="rehearsal on a one-GPU box: every rank renders on GPU 0")
    return p.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    s = render_batch(args, rank, world, 0 if args.all_ranks_on_device0 else local_rank, log=lambda m: print(m, flush=True))
    s["Mpixels_per_s"] = s["frames_rendered"] * args.width * args.height / s["seconds"] / 1e6 if s["seconds"] else 0.0
    s["frames_per_s"] = s["frames_rendered"] / s["seconds"] if s["seconds"] else 0.0
    s["config"] = "%d frames %dx%d %s %d steps, format %s, frame f -> rank f %% %d" % (
        args.frames, args.width, args.height, args.scene, args.max_iter, args.format, world)
    print(json.dumps(s), flush=True)


if __name__ == "__main__":
    main()
