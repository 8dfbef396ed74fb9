"""Overhangs and supports from RayMarchingResources.support_solid: which surfaces of the solid map_scene < level overhang for a
build direction, how much support material they need, where it lands -- on the plate, or on the part, where it leaves scars --
and which of the six axis directions is the cheapest way up.

  python -m ray_marching_amd.supports --scene g32 --lo -2.5 --hi 2.5 --res 256 --up +z
  python -m ray_marching_amd.supports --program part.json --res 512 --up best --max-overhang 50 --regions --fail-on "support>2.5,landings>0"

evaluates a named scene (csg.scene) or a program file (massprops.load_program) on the GPU and prints one JSON line: the build
direction, the squared reach the angle gives (renderer.reach_r2; the box must give one step for the two in-layer axes), the
plate's height, the eight counts, the support volume and the contact area in world units.  --up best runs all six directions
and picks the least support volume; ties break by fewer landings, then by the order +z, -z, +y, -y, +x, -x; the report carries
all six.  --plate H puts the plate at height H (a layer index along the build direction) instead of under the lowest point.
--profile adds the per-layer table (inside, overhang, support on the plate, support on the part).  --mask writes the mask (uint8
[k, j, i]: 0 outside, 1 inside, 2 overhang, 3 support on the plate, 4 support on the part) as a .npy file.  --regions labels the
overhang points and the support points (label_occupancy) and reports each region's points, volume and centre.  --fail-on is a
printability gate: a comma-separated list of `overhang>N`, `landings>N` (points) and `support>V` (world volume); the exit status
is 2 when one holds.  --mesh-out writes the support points (classes 3 and 4 of the mask) as a closed
triangle mesh of unit faces (.stl, .obj or .ply; mesh_classes: DESIGN.md section 29); the report carries its counts under "mesh"."""
import argparse
import json
import re
import sys

from . import lattice_image, lattice_mesh

from .massprops import load_program
from .mesh import _three

GATES = ("overhang", "support", "landings")
BEST_ORDER = ("+z", "-z", "+y", "-y", "+x", "-x")


def parse_gates(text):
    """"overhang>0,support>2.5" -> [("overhang", 0.0), ("support", 2.5)]."""
    gates = []
    for part in filter(None, (p.strip() for p in (text or "").split(","))):
        m = re.fullmatch(r"(\w+)\s*>\s*(-?\d+(?:\.\d*)?(?:[eE][-+]?\d+)?)", part)
        if not m or m.group(1) not in GATES:
            raise ValueError("--fail-on: %r is not one of overhang>N, support>V, landings>N" % part)
        gates.append((m.group(1), float(m.group(2))))
    return gates


def failed_gates(gates, values):
    return ["%s = %g > %g" % (name, values[name], limit) for name, limit in gates if values[name] > limit]


def best_direction(reports):
    """The direction of the least support volume among {up: report}; ties: fewer landings, then BEST_ORDER."""
    return min(reports, key=lambda up: (reports[up]["support"], reports[up]["landings"], BEST_ORDER.index(up)))


def direction_report(res, lo, hi, shape, level, up, angle, plate, want_profile):
    """(report, Support) of one direction."""
    from . import renderer
    _, step, _ = res._box_lattice(lo, hi, shape)
    a = BEST_ORDER.index(up) // 2                                   # 0: z, 1: y, 2: x
    axis = 2 - a
    r2 = renderer.reach_r2(angle, float(step[axis]), [float(step[b]) for b in range(3) if b != axis])
    sup = res.support_solid(lo, hi, shape, level=level, up=up, r2=r2, plate=plate)
    report = dict(sup.counts, up=up, r2=r2, support=sup.volume(), contact_area=sup.contact_area())
    if want_profile:
        report["profile"] = sup.profile().tolist()
    return report, sup


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ray_marching_amd.supports", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32", help="a csg.scene name (g1, g8, g32, g32_balanced, mat_mix, ...)")
    ap.add_argument("--program", default=None, help='a program file instead of --scene: JSON {"cmd_count": n, "words": [...]}')
    ap.add_argument("--lo", default="-2.5", help="lower box corner: one value for all axes, or x,y,z")
    ap.add_argument("--hi", default="2.5", help="upper box corner: one value, or x,y,z")
    ap.add_argument("--res", default="256", help="lattice points per axis (2..1024, at most 2^28 in all): n, or nx,ny,nz")
    ap.add_argument("--level", type=float, default=0.0)
    ap.add_argument("--up", default="+z", choices=BEST_ORDER + ("best",), help="the build direction, or best: the least support volume of the six")
    ap.add_argument("--max-overhang", type=float, default=45.0, help="the largest self-supporting angle from the build direction, degrees")
    ap.add_argument("--plate", type=int, default=None, help="the plate's height (a layer index); default: under the lowest point")
    ap.add_argument("--mask", default=None, help="write the mask to this .npy file")
    ap.add_argument("--profile", action="store_true", help="put the per-layer table into the report")
    ap.add_argument("--regions", action="store_true", help="label the overhang and the support points and report every region")
    ap.add_argument("--fail-on", default="", help='e.g. "overhang>0,support>2.5,landings>0": exit status 2 when one of them holds')
    lattice_image.add_options(ap)
    lattice_mesh.add_options(ap, "supports")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    gates = parse_gates(a.fail_on)
    lattice_mesh.check_path(a.mesh_out)
    import numpy as np
    from . import _ffi, csg, renderer
    res = renderer.RayMarchingResources(a.device)
    try:
        if a.program is not None:
            cc, words = load_program(a.program)
            res.resize_command_buffer(max(1024, 4 * (len(words) + 1)))
            res.set_program(cc, words)
        else:
            res.set_scene(csg.scene(a.scene))
        lo, hi, shape = _three(a.lo, float, "--lo"), _three(a.hi, float, "--hi"), _three(a.res, int, "--res")
        run = lambda up: direction_report(res, lo, hi, shape, a.level, up, a.max_overhang, a.plate, a.profile)   # noqa: E731
        if a.up == "best":
            every = {up: run(up)[0] for up in BEST_ORDER}
            up = best_direction(every)
            report, sup = run(up)                                   # again: only the context's last Support reads
            report["directions"] = every
        else:
            report, sup = run(a.up)
        report.update(shape=list(sup.shape), step=[float(x) for x in sup.step], stats=sup.stats)
        mask = sup.mask() if (a.mask or a.regions) else None
        if a.mask:
            np.save(a.mask, mask)
        if a.regions:
            for key, occ in (("overhang_regions", mask == _ffi.SUP_MASK_OVERHANG), ("support_regions", mask >= _ffi.SUP_MASK_ON_PLATE)):
                regions = []
                if occ.any():
                    for row in res.label_occupancy(occ.astype(np.uint8)).body_moments:
                        p = renderer.mass_from_moments(row, sup.origin, sup.step, 1.0)
                        regions.append({"points": int(row[0]), "volume": p["volume"], "centre": [float(x) for x in p["centroid"]]})
                report[key] = regions
        if a.image:
            cls = lattice_image.device_bytes(res, sup.shape, lambda p, st: res.read_support_device(mask_ptr=p, stream=st))
            report["image"] = lattice_image.write(res, cls, sup.origin, sup.step, a.image, a.size, a.cut)
        if a.mesh_out:                                              # the supports (classes 3 and 4) against everything else
            cls = lattice_image.device_bytes(res, sup.shape, lambda p, st: res.read_support_device(mask_ptr=p, stream=st))
            report["mesh"] = lattice_mesh.write(res, "supports", cls, sup.origin, sup.step, a.mesh_out)
    finally:
        res.close()
    failed = failed_gates(gates, {"overhang": report["overhang"], "support": report["support"], "landings": report["landings"]})
    report["failed"] = failed
    print(json.dumps(report))
    return 2 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
