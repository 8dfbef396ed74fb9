#!/usr/bin/env python3
"""What the pre-pass can know about a frame, counted on the CPU (no GPU): every 8 x 8 tile of a scene / camera / size is put
in one class from binary64 geometry on the primitives the miss-test tables keep (their zones, tests/cull_ref.py) and the numpy
oracle's binary32 rays and floor codes.

  marched          some pixel has a sample ray that meets a zone
  clear            no sample ray of the tile meets a zone: the pre-pass finishes the tile
    sky            ... and all 1024 samples are black
    one cell       ... and all 1024 samples fall in one checker cell
    mixed          ... the horizon, cell edges: some pixels need their samples looked at one by one
  clear by the tile test   the tile's centre ray misses every zone inflated by 2 rho D (rho the tile's angular radius, D the far
                   end of the zone from the camera): a model of a whole-tile test with generous slack
  settled          clear by the tile test and sky or one cell: what a per-tile decision can finish

and, inside the marched tiles, how much a march kernel could skip: the share of rays, pixels and 2 x 2 pixel batches that are
provably clear.  Prints the table and writes a JSON file (--out; by default only the metric frame's, into profiles/).

The zones are the tables' own: every primitive grown by cull_margin (about 0.011 for the metric frame).  The count the tile
verdicts were first priced with used a fixed margin of 0.02 (--margin 0.02) and a coarser sky test, and found 7 688 marched /
24 712 clear / 16 949 sky tiles where this tool finds 7 499 / 24 901 / 18 661; hits, step counts and wave iterations of the
marched rays were part of that one-off count and are not computed here.

usage: tools/prepass_tile_classes.py [--scene g32] [--camera still|orbitN] [--width 1920 --height 1080] [--margin M]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

F = np.float32
OUT = os.path.join(ROOT, "profiles", "r11_prepass_tile_classes.json")


def uniforms(camera_name, W, H):
    import math
    from ray_marching_amd import camera, renderer
    ctl = camera.OrbitCameraController.new([0.0, 0.0, 0.0], 5.0)
    if camera_name == "still":
        ctl.update(camera.Orbit([35.0, -25.0]))
    else:                                               # frame N of the 1024-frame orbit batch
        ctl.set_angles(2.0 * math.pi * int(camera_name[5:]) / 1024, -0.25, 5.0)
    u = renderer.prepare_uniforms((W, H), ctl.camera())
    return {"viewport_extent": list(u.viewport_extent), "inv_proj": list(u.inv_proj), "inv_view": list(u.inv_view)}


def zones_of(cc, words, ro, min_dist, margin):
    import cull_ref as R
    from test_cull_tables_cpu import KIND_TO_OP, N_PARAMS, decode
    d = decode(cc, words)
    slack = float(F(d["smooth_slack"]))
    out = []
    for r in d["rec"]:
        if r["kind"] not in (1, 2, 3) or r["nocull"]:
            continue
        z = (R.zone(R.SPHERE, d["bounds"][r["slot"]], ro, min_dist, slack) if d["has_xforms"]
             else R.zone(KIND_TO_OP[r["kind"]], r["p"][:N_PARAMS[r["kind"]]], ro, min_dist, slack))
        if margin is not None:                          # a fixed margin instead of the device's cull_margin
            m0 = R.cull_margin(z[1], z[2] if z[0] == "ball" else np.sum(z[2]), ro, min_dist, slack)
            z = (z[0], z[1], z[2] - m0 + margin)
        out.append(z)
    return out


def floor_cells(ro, d):
    """(ix, iz) of the floor cell a miss ray lands in, as the oracle computes them; sky: ix = iz = INT64_MIN."""
    from oracle import rm_oracle_np as onp
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        fd = (F(-1.5) - ro[1]) / d[1]
        on = fd > 0
        ix = onp.f2i(np.rint((ro[0] + d[0] * fd) + F(0.5))).astype(np.int64)
        iz = onp.f2i(np.rint((ro[2] + d[2] * fd) + F(0.5))).astype(np.int64)
    sky = np.iinfo(np.int64).min
    return np.where(on, ix, sky), np.where(on, iz, sky)


def classify(scene, camera_name, W, H, min_dist, margin):
    import cull_ref as R
    import gbuffer_ref
    from ray_marching_amd import csg
    cc, words = csg.serialize(csg.scene(scene))
    ud = uniforms(camera_name, W, H)
    ro4, _ = gbuffer_ref.camera_rays(np.zeros(1, np.uint32), np.zeros(1, np.uint32), 0, ud, W, H)
    ro = np.array(ro4, dtype=F)[:3]
    ro64 = ro.astype(np.float64)
    zones = zones_of(cc, np.asarray(words, dtype=np.uint32), ro64, min_dist, margin)
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    n = {k: 0 for k in ("tiles", "marched", "clear", "sky", "one_cell", "mixed", "mixed_le_24", "mixed_pixels", "tile_test_clear", "settled",
                        "marched_rays", "marched_rays_clear", "marched_pixels", "marched_pixels_clear", "marched_batches", "marched_batches_clear")}
    for ty in range(tiles_y):                            # one row of tiles at a time: (8 rows x W) pixels x 16 samples
        rows = np.arange(ty * 8, min(ty * 8 + 8, H))
        px, py = np.meshgrid(np.arange(W, dtype=np.uint32), rows.astype(np.uint32))
        px, py = px.ravel(), py.ravel()
        meets = np.zeros((16, len(px)), dtype=bool)
        ix, iz = np.zeros((16, len(px)), dtype=np.int64), np.zeros((16, len(px)), dtype=np.int64)
        dirs = {}
        for s in range(16):
            _, d = gbuffer_ref.camera_rays(px, py, s, ud, W, H)
            d64 = np.stack(d, axis=1).astype(np.float64)
            for z in zones:
                meets[s] |= R.meets_zone(z, ro64, d64)
            ix[s], iz[s] = floor_cells(ro, d)
            if s in (0, 3, 12, 15):
                dirs[s] = d64
        tile = px // 8
        pixel_clear = ~meets.any(axis=0)
        pending = np.bincount(tile, weights=~pixel_clear, minlength=tiles_x)
        one_colour = (ix.min(axis=0) == ix.max(axis=0)) & (iz.min(axis=0) == iz.max(axis=0))          # per pixel
        lo = lambda a: np.array([a[:, tile == t].min() for t in range(tiles_x)])                       # noqa: E731
        hi = lambda a: np.array([a[:, tile == t].max() for t in range(tiles_x)])                       # noqa: E731
        uniform = (lo(ix) == hi(ix)) & (lo(iz) == hi(iz))
        is_sky = uniform & (hi(ix) == np.iinfo(np.int64).min)
        need = np.bincount(tile, weights=~one_colour, minlength=tiles_x)
        # the whole-tile test: the four extreme samples of the tile span its cone
        last = len(rows) - 1
        cone_ok = np.zeros(tiles_x, dtype=bool)
        for t in range(tiles_x):
            x0, x1 = t * 8, min(t * 8 + 7, W - 1)
            e = np.array([dirs[0][x0], dirs[12][x1], dirs[3][last * W + x0], dirs[15][last * W + x1]])
            c = e.sum(axis=0)
            c /= np.linalg.norm(c)
            rho = np.linalg.norm(e - c, axis=1).max()
            ok = True
            for z in zones:
                D = np.linalg.norm(z[1] - ro64) + (z[2] if z[0] == "ball" else np.linalg.norm(z[2]))
                ok = ok and not R.meets_zone((z[0], z[1], z[2] + 2.0 * rho * D), ro64, c[None, :])[0]
            cone_ok[t] = ok
        marched = pending > 0
        n["tiles"] += tiles_x
        n["marched"] += int(marched.sum())
        n["clear"] += int((~marched).sum())
        n["sky"] += int((~marched & is_sky).sum())
        n["one_cell"] += int((~marched & uniform & ~is_sky).sum())
        mixed = ~marched & ~uniform
        n["mixed"] += int(mixed.sum())
        n["mixed_le_24"] += int((mixed & (need <= 24)).sum())
        n["mixed_pixels"] += int(need[mixed].sum())
        n["tile_test_clear"] += int(cone_ok.sum())
        n["settled"] += int((cone_ok & uniform).sum())
        in_marched = marched[tile]
        n["marched_rays"] += 16 * int(in_marched.sum())
        n["marched_rays_clear"] += int((~meets[:, in_marched]).sum())
        n["marched_pixels"] += int(in_marched.sum())
        n["marched_pixels_clear"] += int(pixel_clear[in_marched].sum())
        if len(rows) == 8 and W % 2 == 0:
            b = pixel_clear.reshape(4, 2, W // 2, 2).all(axis=(1, 3)) & in_marched.reshape(4, 2, W // 2, 2)[:, 0, :, 0]
            n["marched_batches"] += int(in_marched.sum()) // 4
            n["marched_batches_clear"] += int(b.sum())
        if sys.stderr.isatty():
            print("tile row %d / %d" % (ty + 1, tiles_y), end="\r", file=sys.stderr, flush=True)
    return {"scene": scene, "camera": camera_name, "frame": [W, H], "min_dist": min_dist, "margin": margin, "kept_primitives": len(zones), "counts": n}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32")
    ap.add_argument("--camera", default="still", help="still, or orbitN: frame N of the 1024-frame orbit")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--min-dist", type=float, default=0.01)
    ap.add_argument("--margin", type=float, default=None, help="fixed margin around the primitives (default: the tables' own)")
    ap.add_argument("--out", default=None, help="JSON file; default: profiles/r11_prepass_tile_classes.json for the metric frame "
                    "(every other argument at its default), none otherwise")
    a = ap.parse_args()
    if a.out is None and all(getattr(a, k) == ap.get_default(k) for k in ("scene", "camera", "width", "height", "min_dist", "margin")):
        a.out = OUT
    res = classify(a.scene, a.camera, a.width, a.height, a.min_dist, a.margin)
    n = res["counts"]
    for k in ("marched", "clear", "sky", "one_cell", "mixed", "tile_test_clear", "settled"):
        print("%-16s %6d  %5.1f %%" % (k, n[k], 100.0 * n[k] / n["tiles"]))
    print("mixed tiles with <= 24 pixels to sample: %d; pixels to sample: %d" % (n["mixed_le_24"], n["mixed_pixels"]))
    for k in ("rays", "pixels", "batches"):
        print("marched tiles: %.1f %% of the %s are provably clear" % (100.0 * n["marched_%s_clear" % k] / max(n["marched_%s" % k], 1), k))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
