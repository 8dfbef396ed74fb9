"""Mass properties from RayMarchingResources.mass_properties: volume, mass, centre of mass, inertia tensor and bounding box of
the solid map_scene < level, from exact integer moments of its occupancy lattice.

  python -m ray_marching_amd.massprops --scene g32 --lo -2.5 --hi 2.5 --res 512 --density 7.85
  python -m ray_marching_amd.massprops --program part.json --lo -1,-1,0 --hi 1,1,2 --res 1024,1024,512

evaluates a named scene (csg.scene) or a program file on the GPU and prints one JSON object: properties, moments and stats.  A
program file is JSON: {"cmd_count": n, "words": [...]} (what csg.serialize returns).  A first-order quadrature (each inside
lattice point stands for its cell); the moments themselves are exact."""
import argparse
import json
import sys

from .mesh import _three


def load_program(path):
    """(cmd_count, words) of a program file."""
    with open(path) as f:
        p = json.load(f)
    return int(p["cmd_count"]), [int(w) for w in p["words"]]


def report(props):
    """mass_properties' dict as plain JSON types."""
    from . import _ffi
    inertia = props["inertia"]
    return {
        "properties": {"volume": props["volume"], "mass": props["mass"], "centroid": [float(x) for x in props["centroid"]],
                       "inertia": [[float(x) for x in row] for row in inertia],
                       "bbox_lo": [float(x) for x in props["bbox_lo"]], "bbox_hi": [float(x) for x in props["bbox_hi"]]},
        "moments": [int(x) for x in props["moments"][:_ffi.RM_MOMENTS]],
        "stats": dict(props["stats"]),
    }


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ray_marching_amd.massprops", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32", help="a csg.scene name (g1, g8, g32, g32_balanced, mat_mix, ...)")
    ap.add_argument("--program", default=None, help='a program file instead of --scene: JSON {"cmd_count": n, "words": [...]}')
    ap.add_argument("--lo", default="-3", help="lower box corner: one value for all axes, or x,y,z")
    ap.add_argument("--hi", default="3", help="upper box corner: one value, or x,y,z")
    ap.add_argument("--res", default="256", help="lattice points per axis (2..4096): n, or nx,ny,nz")
    ap.add_argument("--level", type=float, default=0.0)
    ap.add_argument("--density", type=float, default=1.0, help="mass per unit volume")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    from . import csg, renderer
    res = renderer.RayMarchingResources(a.device)
    try:
        if a.program is not None:
            cc, words = load_program(a.program)
            res.resize_command_buffer(max(1024, 4 * (len(words) + 1)))
            res.set_program(cc, words)
        else:
            res.set_scene(csg.scene(a.scene))
        props = res.mass_properties(_three(a.lo, float, "--lo"), _three(a.hi, float, "--hi"), _three(a.res, int, "--res"), level=a.level,
                                    density=a.density)
    finally:
        res.close()
    print(json.dumps(report(props)))


if __name__ == "__main__":
    sys.exit(main())
