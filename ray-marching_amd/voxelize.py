"""Printability checks for a part that arrives as a triangle mesh: RayMarchingResources.voxelize_mesh_box turns an STL, OBJ or PLY
file into the occupancy of a lattice on the GPU, and the lattice analyses take that occupancy without it leaving the device.

  python -m ray_marching_amd.voxelize bracket.stl --res 256
  python -m ray_marching_amd.voxelize bracket.stl --res 512 --report topology,thickness --fail-on "open_rows>0,rejected>0,bodies>1"

reads the file (mesh.read), voxelises it on a lattice of --res points along the longest axis of its bounding box with --margin
empty points all round (one step for all three axes), and prints one JSON object: the voxel counts (triangles, rejected, edge_on,
crossings, inside, open_rows: open_rows > 0 means that the mesh is not closed), the lattice, and per name of --report the counts of
that analysis of the occupancy: topology (label_occupancy), thickness (distance_occupancy, with the inscribed radius in world
units), supports and islands (support_occupancy, islands_occupancy for --up and --r2), surface (surface_classes: the area of the
voxel solid).  --out writes the occupancy as a .npy file, uint8 indexed [k, j, i].  --fail-on is a gate: a comma-separated list
of `name>N` or `name<N` over the voxel counts and the counts of the requested reports (`report.name` where two reports share a
name); the exit status is 2 when one holds.  --image writes a picture of the voxel solid (a PNG of --size,
through an orbit camera aimed at the lattice's box; --cut axis:lo:hi shows only that slab of lattice points: DESIGN.md section 28).
--mesh-out writes the voxel solid as a closed triangle mesh of unit faces (.stl, .obj or .ply; mesh_classes: DESIGN.md section 29);
the report carries its counts under "mesh"."""
import argparse
import json
import re
import sys

import numpy as np

from . import _ffi, lattice_image, lattice_mesh

REPORTS = {"topology": _ffi.TOPO_COUNT_NAMES, "thickness": _ffi.DIST_COUNT_NAMES + ("inscribed_radius",),
           "supports": _ffi.SUP_COUNT_NAMES, "islands": _ffi.ISL_COUNT_NAMES, "surface": _ffi.SURF_MEASURE_NAMES}
UPS = _ffi.UP_NAMES


def parse_reports(text):
    """"topology,thickness" -> ["topology", "thickness"]."""
    names = [p.strip() for p in (text or "").split(",") if p.strip()]
    for name in names:
        if name not in REPORTS:
            raise ValueError("--report: %r is not one of %s" % (name, ", ".join(REPORTS)))
    return names


def parse_gates(text, reports=()):
    """"open_rows>0,bodies>1,inscribed_radius<0.4" -> [("open_rows", ">", 0.0), ...].  A name is a voxel count, a count of one of
    `reports`, or report.count."""
    known = set(_ffi.VOX_COUNT_NAMES)
    for r in reports:
        known |= set(REPORTS[r]) | {"%s.%s" % (r, n) for n in REPORTS[r]}
    gates = []
    for part in filter(None, (p.strip() for p in (text or "").split(","))):
        m = re.fullmatch(r"([\w.]+)\s*([<>])\s*(-?\d+(?:\.\d*)?(?:[eE][-+]?\d+)?)", part)
        if not m:
            raise ValueError("--fail-on: %r is not name>N or name<N" % part)
        if m.group(1) not in known:
            raise ValueError("--fail-on: %r is not a voxel count (%s) nor a count of a requested report" % (m.group(1), ", ".join(_ffi.VOX_COUNT_NAMES)))
        gates.append((m.group(1), m.group(2), float(m.group(3))))
    return gates


def gate_values(report, reports):
    """name -> value for the gates: the voxel counts, each report's counts as report.name, and by the bare name from the first
    report that has it."""
    values = dict(report["voxels"])
    for r in reports:
        for name, v in report[r].items():
            if isinstance(v, (int, float)) and v == v:
                values["%s.%s" % (r, name)] = v
                values.setdefault(name, v)
    return values


def failed_gates(gates, values):
    return ["%s = %g %s %g" % (name, values[name], op, limit) for name, op, limit in gates
            if name in values and (values[name] > limit if op == ">" else values[name] < limit)]


def analyse(res, vox, reports, up, r2):
    """The counts of each requested analysis of the device occupancy of `vox`."""
    occ = vox.occupancy_device()
    out = {}
    for name in reports:
        if name == "topology":
            out[name] = res.label_occupancy(occ).counts
        elif name == "thickness":
            d = res.distance_occupancy(occ)
            out[name] = dict(d.counts, inscribed_radius=d.inscribed_radius(vox.step)[0])
        elif name == "supports":
            out[name] = res.support_occupancy(occ, up=up, r2=r2).counts
        elif name == "islands":
            out[name] = res.islands_occupancy(occ, up=up, r2=r2).counts
        elif name == "surface":
            m = res.surface_classes(occ).measures(1, 0, vox.step)
            out[name] = {k: (None if v != v else v) for k, v in m.items()}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ray_marching_amd.voxelize", description=__doc__.split("\n\n")[0])
    ap.add_argument("file", help="a mesh file: .stl, .obj or .ply")
    ap.add_argument("--res", type=int, default=128, help="lattice points along the longest axis of the bounding box (at most 1024)")
    ap.add_argument("--margin", type=int, default=2, help="empty lattice points round the bounding box")
    ap.add_argument("--out", default=None, help="write the occupancy here (.npy, uint8 [k, j, i])")
    ap.add_argument("--report", default="", help="analyses of the occupancy: a comma-separated list of " + ", ".join(REPORTS))
    ap.add_argument("--up", default="+z", choices=UPS, help="the build direction of supports and islands")
    ap.add_argument("--r2", type=int, default=1, help="the squared reach of supports and islands (index units, 0..255)")
    ap.add_argument("--fail-on", default="", help='e.g. "open_rows>0,rejected>0,bodies>1": exit status 2 when one of them holds')
    lattice_image.add_options(ap)
    lattice_mesh.add_options(ap, "voxelize")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    lattice_mesh.check_path(a.mesh_out)
    try:
        reports = parse_reports(a.report)
        gates = parse_gates(a.fail_on, reports)
    except ValueError as e:
        ap.error(str(e))
    from . import mesh, renderer
    m = mesh.read(a.file)
    res = renderer.RayMarchingResources(a.device)
    try:
        vox = res.voxelize_mesh_box(m.vertices, m.triangles, a.res, a.margin)
        report = {"file": a.file, "vertices": len(m.vertices), "voxels": vox.counts, "shape": list(vox.shape),
                  "origin": [float(x) for x in vox.origin], "step": [float(x) for x in vox.step], "stats": vox.stats}
        report.update(analyse(res, vox, reports, a.up, a.r2))
        if a.out:
            np.save(a.out, vox.occupancy())
        if a.image:                                              # the occupancy never leaves the device
            report["image"] = lattice_image.write(res, vox.occupancy_device(), vox.origin, vox.step, a.image, a.size, a.cut)
        if a.mesh_out:
            report["mesh"] = lattice_mesh.write(res, "voxelize", vox.occupancy_device(), vox.origin, vox.step, a.mesh_out)
    finally:
        res.close()
    report["failed"] = failed_gates(gates, gate_values(report, reports))
    print(json.dumps(report))
    return 2 if report["failed"] else 0


if __name__ == "__main__":
    sys.exit(main())
