"""Solid topology from RayMarchingResources.label_solid: is the part one piece, does it enclose voids, does it have
through-holes -- bodies, cavities and tunnels of the solid map_scene < level on a lattice, with the mass properties of every body.

  python -m ray_marching_amd.topology --scene g32 --lo -2.5 --hi 2.5 --res 256
  python -m ray_marching_amd.topology --program part.json --res 512 --labels labels.npy --fail-on "bodies>1,cavities>0"

evaluates a named scene (csg.scene) or a program file (massprops.load_program) on the GPU and prints a report: every body with
its volume, centre and box, every cavity with its volume and box, the tunnels and the Euler characteristic.  --labels writes the
label volume (uint32 [k, j, i]: a body's number, 0x80000000 | a cavity's number, 0xFFFFFFFF for the exterior).  --fail-on is a
printability gate: a comma-separated list of `name>limit` over bodies, cavities and tunnels; the exit status is 2 when one holds.
Bodies are connected through faces, voids through faces, edges and corners."""
import argparse
import re
import sys

from .massprops import load_program
from .mesh import _three

GATE_NAMES = ("bodies", "cavities", "tunnels")


def parse_gates(text):
    """"bodies>1,cavities>0" -> [("bodies", 1), ("cavities", 0)]."""
    gates = []
    for part in filter(None, (p.strip() for p in (text or "").split(","))):
        m = re.fullmatch(r"(\w+)\s*>\s*(-?\d+)", part)
        if not m or m.group(1) not in GATE_NAMES:
            raise ValueError("--fail-on: %r is not `name>limit` with a name of %s" % (part, ", ".join(GATE_NAMES)))
        gates.append((m.group(1), int(m.group(2))))
    return gates


def failed_gates(gates, counts):
    return ["%s = %d > %d" % (name, counts[name], limit) for name, limit in gates if counts[name] > limit]


def report_lines(topo, density=1.0):
    """The report of a renderer.Topology, one line per entry."""
    fmt3 = lambda v: "(%s)" % ", ".join("%.6g" % float(x) for x in v)  # noqa: E731
    lines = ["lattice %s: %d bodies, %d cavities, %d tunnels, Euler characteristic %d"
             % ("x".join(map(str, topo.shape)), topo.bodies, topo.cavities, topo.tunnels, topo.euler)]
    for b, p in enumerate(topo.body_properties(density)):
        lines.append("body %d: volume %.6g, mass %.6g, centre %s, box %s .. %s"
                     % (b, p["volume"], p["mass"], fmt3(p["centroid"]), fmt3(p["bbox_lo"]), fmt3(p["bbox_hi"])))
    for c, p in enumerate(topo.cavity_properties()):
        lines.append("cavity %d: volume %.6g, box %s .. %s" % (c, p["volume"], fmt3(p["bbox_lo"]), fmt3(p["bbox_hi"])))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ray_marching_amd.topology", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32", help="a csg.scene name (g1, g8, g32, g32_balanced, mat_mix, ...)")
    ap.add_argument("--program", default=None, help='a program file instead of --scene: JSON {"cmd_count": n, "words": [...]}')
    ap.add_argument("--lo", default="-2.5", help="lower box corner: one value for all axes, or x,y,z")
    ap.add_argument("--hi", default="2.5", help="upper box corner: one value, or x,y,z")
    ap.add_argument("--res", default="256", help="lattice points per axis (2..1024, at most 2^28 in all): n, or nx,ny,nz")
    ap.add_argument("--level", type=float, default=0.0)
    ap.add_argument("--density", type=float, default=1.0, help="mass per unit volume")
    ap.add_argument("--labels", default=None, help="write the label volume to this .npy file")
    ap.add_argument("--fail-on", default="", help='e.g. "bodies>1,cavities>0": exit status 2 when one of them holds')
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    gates = parse_gates(a.fail_on)
    from . import csg, renderer
    res = renderer.RayMarchingResources(a.device)
    try:
        if a.program is not None:
            cc, words = load_program(a.program)
            res.resize_command_buffer(max(1024, 4 * (len(words) + 1)))
            res.set_program(cc, words)
        else:
            res.set_scene(csg.scene(a.scene))
        topo = res.label_solid(_three(a.lo, float, "--lo"), _three(a.hi, float, "--hi"), _three(a.res, int, "--res"), level=a.level)
        print("\n".join(report_lines(topo, a.density)))
        if a.labels:
            import numpy as np
            np.save(a.labels, topo.labels())
    finally:
        res.close()
    failed = failed_gates(gates, topo.counts)
    for f in failed:
        print("FAIL: %s" % f)
    return 2 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
