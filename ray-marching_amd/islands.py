"""Layer regions and islands from RayMarchingResources.islands_solid: for a build direction, how many separate regions every layer
of the solid map_scene < level has, where regions merge, and which regions start printing in mid air -- the islands that lose a
part on a resin or a powder machine.

  python -m ray_marching_amd.islands --scene g32 --lo -2.5 --hi 2.5 --res 256 --up +z
  python -m ray_marching_amd.islands --program part.json --res 512 --up best --max-overhang 50 --rows --fail-on "islands>0,layer_regions>40"

evaluates a named scene (csg.scene) or a program file (massprops.load_program) on the GPU and prints one JSON line: the build
direction, the squared reach the angle gives (renderer.reach_r2; the box must give one step for the two in-layer axes), the eight
counts, and every island with its layer, points, centroid and area in world units.  --up best runs all six directions and picks
the fewest islands; ties break by fewer island points, then by the order +z, -z, +y, -y, +x, -x; the report carries all six.
--plate H puts the plate at height H (a layer index along the build direction) instead of under the lowest point.  --rows adds the
region table (one list of twelve numbers per region, _ffi.ISL_ROW_NAMES) and for every region the island or base region it grows
from; --profile the per-layer table (inside points, regions, islands, island points).  --mask writes the mask (uint8 [k, j, i]: 0
outside, 1 inside, 2 inside and in an island) and --labels the label volume (uint32 [k, j, i]) as .npy files.  --fail-on is a
printability gate: a comma-separated list of `islands>N`, `island_points>N` and `layer_regions>N` (the most regions in one layer);
the exit status is 2 when one holds.  --mesh-out writes the island points (class 2 of the mask) as a closed
triangle mesh of unit faces (.stl, .obj or .ply; mesh_classes: DESIGN.md section 29); the report carries its counts under "mesh"."""
import argparse
import json
import re
import sys

from . import lattice_image, lattice_mesh

from .massprops import load_program
from .mesh import _three

GATES = ("islands", "island_points", "layer_regions")
BEST_ORDER = ("+z", "-z", "+y", "-y", "+x", "-x")


def parse_gates(text):
    """"islands>0,layer_regions>40" -> [("islands", 0.0), ("layer_regions", 40.0)]."""
    gates = []
    for part in filter(None, (p.strip() for p in (text or "").split(","))):
        m = re.fullmatch(r"(\w+)\s*>\s*(-?\d+(?:\.\d*)?(?:[eE][-+]?\d+)?)", part)
        if not m or m.group(1) not in GATES:
            raise ValueError("--fail-on: %r is not one of islands>N, island_points>N, layer_regions>N" % part)
        gates.append((m.group(1), float(m.group(2))))
    return gates


def failed_gates(gates, values):
    return ["%s = %g > %g" % (name, values[name], limit) for name, limit in gates if values[name] > limit]


def gate_values(counts):
    """The numbers the gates test, from the counts of a report."""
    return {"islands": counts["islands"], "island_points": counts["island_points"], "layer_regions": counts["max_layer_regions"]}


def best_direction(reports):
    """The direction of the fewest islands among {up: report}; ties: fewer island points, then BEST_ORDER."""
    return min(reports, key=lambda up: (reports[up]["islands"], reports[up]["island_points"], BEST_ORDER.index(up)))


def direction_report(res, lo, hi, shape, level, up, angle, plate):
    """(report, Islands) of one direction."""
    from . import renderer
    _, step, _ = res._box_lattice(lo, hi, shape)
    axis = 2 - BEST_ORDER.index(up) // 2
    r2 = renderer.reach_r2(angle, float(step[axis]), [float(step[b]) for b in range(3) if b != axis])
    isl = res.islands_solid(lo, hi, shape, level=level, up=up, r2=r2, plate=plate)
    return dict(isl.counts, up=up, r2=r2), isl


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ray_marching_amd.islands", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32", help="a csg.scene name (g1, g8, g32, g32_balanced, mat_mix, ...)")
    ap.add_argument("--program", default=None, help='a program file instead of --scene: JSON {"cmd_count": n, "words": [...]}')
    ap.add_argument("--lo", default="-2.5", help="lower box corner: one value for all axes, or x,y,z")
    ap.add_argument("--hi", default="2.5", help="upper box corner: one value, or x,y,z")
    ap.add_argument("--res", default="256", help="lattice points per axis (2..1024, at most 2^28 in all): n, or nx,ny,nz")
    ap.add_argument("--level", type=float, default=0.0)
    ap.add_argument("--up", default="+z", choices=BEST_ORDER + ("best",), help="the build direction, or best: the fewest islands of the six")
    ap.add_argument("--max-overhang", type=float, default=45.0, help="the largest self-supporting angle from the build direction, degrees")
    ap.add_argument("--plate", type=int, default=None, help="the plate's height (a layer index); default: under the lowest point")
    ap.add_argument("--mask", default=None, help="write the mask to this .npy file")
    ap.add_argument("--labels", default=None, help="write the label volume to this .npy file")
    ap.add_argument("--rows", action="store_true", help="put the region table and every region's root into the report")
    ap.add_argument("--profile", action="store_true", help="put the per-layer table into the report")
    ap.add_argument("--fail-on", default="", help='e.g. "islands>0,island_points>0,layer_regions>40": exit status 2 when one of them holds')
    lattice_image.add_options(ap)
    lattice_mesh.add_options(ap, "islands")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    gates = parse_gates(a.fail_on)
    lattice_mesh.check_path(a.mesh_out)
    import numpy as np
    from . import csg, renderer
    res = renderer.RayMarchingResources(a.device)
    try:
        if a.program is not None:
            cc, words = load_program(a.program)
            res.resize_command_buffer(max(1024, 4 * (len(words) + 1)))
            res.set_program(cc, words)
        else:
            res.set_scene(csg.scene(a.scene))
        lo, hi, shape = _three(a.lo, float, "--lo"), _three(a.hi, float, "--hi"), _three(a.res, int, "--res")
        run = lambda up: direction_report(res, lo, hi, shape, a.level, up, a.max_overhang, a.plate)   # noqa: E731
        if a.up == "best":
            every = {up: run(up)[0] for up in BEST_ORDER}
            report, isl = run(best_direction(every))                # again: only the context's last Islands reads
            report["directions"] = every
        else:
            report, isl = run(a.up)
        rows = isl.rows()
        report.update(shape=list(isl.shape), step=[float(x) for x in isl.step], stats=isl.stats, island_list=isl.islands(rows))
        if a.rows:
            report["rows"] = rows.view(np.uint32).reshape(len(rows), -1).tolist()
            report["roots"] = isl.roots(rows).tolist()
        if a.profile:
            report["profile"] = isl.profile().tolist()
        if a.mask:
            np.save(a.mask, isl.mask())
        if a.labels:
            np.save(a.labels, isl.labels())
        if a.image:
            cls = lattice_image.device_bytes(res, isl.shape, lambda p, st: res.read_islands_device(mask_ptr=p, stream=st))
            report["image"] = lattice_image.write(res, cls, isl.origin, isl.step, a.image, a.size, a.cut)
        if a.mesh_out:                                              # the island points (class 2) against everything else
            cls = lattice_image.device_bytes(res, isl.shape, lambda p, st: res.read_islands_device(mask_ptr=p, stream=st))
            report["mesh"] = lattice_mesh.write(res, "islands", cls, isl.origin, isl.step, a.mesh_out)
    finally:
        res.close()
    failed = failed_gates(gates, gate_values(report))
    report["failed"] = failed
    print(json.dumps(report))
    return 2 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
