"""Meshes of class lattices for the command lines: what voxelize, thickness, supports and islands share for --mesh-out.  A
lattice of class bytes (an occupancy, or an analysis' mask: 0 outside, 1 inside, 2.. what the analysis found) is handed to
RayMarchingResources.mesh_classes without leaving the device; the interface between the tool's classes and everything else comes
back as a closed, welded triangle mesh of unit faces and is written by mesh.write as .stl, .obj or .ply."""
from . import mesh

# The classes each tool exports, against every other class.
EXPORTS = {"voxelize": (1,), "thickness": (2, 3), "supports": (3, 4), "islands": (2,)}
EXPORT_NAMES = {"voxelize": "the voxel solid", "thickness": "the thin and the narrow points", "supports": "the supports", "islands": "the islands"}
FORMATS = ("stl", "obj", "ply")


def add_options(ap, tool):
    ap.add_argument("--mesh-out", default=None, metavar="FILE", help="write %s as a triangle mesh here (.stl, .obj or .ply)" % EXPORT_NAMES[tool])


def check_path(path):
    """Refuses a file name mesh.write would refuse, before any work."""
    if path is not None and path.lower().rsplit(".", 1)[-1] not in FORMATS:
        raise SystemExit("--mesh-out: %r is not a .stl, .obj or .ply file" % (path,))


def write(res, tool, classes, origin, step, path):
    """mesh_classes(classes, the tool's classes) written to `path`.  Returns what a report says about the mesh: the file and the
    counts of rm_mesh_classes."""
    m = res.mesh_classes(classes, EXPORTS[tool], None, origin, step)
    mesh.write(m, path)
    return dict(m.counts, file=path, classes=list(EXPORTS[tool]))
