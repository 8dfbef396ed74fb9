"""Surface measures from RayMarchingResources.surface_solid: the surface area of the solid map_scene < level, its staircase
areas by orientation, its volume-to-area ratio -- and, for a build direction, how much area the supports touch the part with,
how large the down-facing overhang skin is and how large the plate footprint.

  python -m ray_marching_amd.surface --scene g1 --lo -2.5 --hi 2.5 --res 256
  python -m ray_marching_amd.surface --program part.json --res 512 --supports --up +z --r2 1 --fail-on "area>40,contact>0.5"

evaluates a named scene (csg.scene) or a program file (massprops.load_program) on the GPU and prints one JSON line: area (the
Cauchy-Crofton estimate of rm_surface_measures; null unless the box gives three equal steps), facet_area and the six facet areas
by orientation (exact areas of the staircase surface, world units), the volume (mass_moments) and volume / area.  --supports runs
support_solid for --up and the squared reach --r2, feeds its mask (0 outside, 1 inside, 2 overhang, 3 support on the plate, 4
support on the part) to surface_classes and adds: contact, the area over which supports touch the part across a layer (the
faces between {1, 2} and {3, 4} along the build axis: the tops under overhangs and the feet on the part); contact_facet_area and
contact_area, the whole part-support interface, sides included, as staircase area and as estimate; overhang_skin, the down-facing
faces of the overhang points; footprint, the area of the part's layer on the plate.  --fail-on is a gate: a comma-separated list
of `area>A` and `contact>A` (world units); the exit status is 2 when one holds."""
import argparse
import json
import math
import re
import sys

from .massprops import load_program
from .mesh import _three

GATES = ("area", "contact")
UPS = ("+x", "-x", "+y", "-y", "+z", "-z")
PART, SUPPORT, OVERHANG, BELOW = (1, 2), (3, 4), (2,), (0, 3, 4)


def parse_gates(text):
    """"area>40,contact>0.5" -> [("area", 40.0), ("contact", 0.5)]."""
    gates = []
    for part in filter(None, (p.strip() for p in (text or "").split(","))):
        m = re.fullmatch(r"(\w+)\s*>\s*(-?\d+(?:\.\d*)?(?:[eE][-+]?\d+)?)", part)
        if not m or m.group(1) not in GATES:
            raise ValueError("--fail-on: %r is not one of area>A, contact>A" % part)
        gates.append((m.group(1), float(m.group(2))))
    return gates


def failed_gates(gates, values):
    return ["%s = %g > %g" % (name, values[name], limit) for name, limit in gates if name in values and values[name] > limit]


def _json_number(x):
    return None if isinstance(x, float) and math.isnan(x) else x


def solid_report(res, lo, hi, shape, level):
    """The report of the solid alone, and the lattice's step."""
    surf = res.surface_solid(lo, hi, shape, level=level)
    m = surf.measures(1, 0)
    volume = res.mass_moments(surf.origin, surf.step, surf.shape, level).properties()["volume"]
    report = {"points": int(surf.points[1]), "volume": volume, "area": m["area"], "facet_area": m["facet_area"],
              "facets": {k[len("facet_"):]: m[k] for k in m if k.startswith("facet_") and k != "facet_area"},
              "volume_area_ratio": volume / m["area"] if m["area"] > 0.0 else None,
              "shape": list(surf.shape), "step": [float(x) for x in surf.step], "stats": surf.stats}
    return report, surf.step


def supports_report(res, lo, hi, shape, level, up, r2, step):
    """What the support mask's pair counts add for the build direction `up`."""
    sup = res.support_solid(lo, hi, shape, level=level, up=up, r2=r2)
    surf = res.surface_classes(sup.mask())
    axis, neg = "xyz"[UPS.index(up) // 2], UPS.index(up) % 2 == 1
    touch = surf.measures(PART, SUPPORT, step)
    skin = surf.measures(OVERHANG, BELOW, step)
    cell = math.prod(float(s) for k, s in enumerate(step) if k != UPS.index(up) // 2)     # the area of a cell of a layer
    return {"up": up, "r2": int(r2), "support_counts": sup.counts,
            "contact": touch["facet_pos_" + axis] + touch["facet_neg_" + axis],
            "contact_facet_area": touch["facet_area"], "contact_area": touch["area"],
            "overhang_skin": skin["facet_pos_" + axis if neg else "facet_neg_" + axis],
            "footprint": sup.counts["base"] * cell}


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ray_marching_amd.surface", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g1", help="a csg.scene name (g1, g8, g32, g32_balanced, mat_mix, ...)")
    ap.add_argument("--program", default=None, help='a program file instead of --scene: JSON {"cmd_count": n, "words": [...]}')
    ap.add_argument("--lo", default="-2.5", help="lower box corner: one value for all axes, or x,y,z")
    ap.add_argument("--hi", default="2.5", help="upper box corner: one value, or x,y,z")
    ap.add_argument("--res", default="256", help="lattice points per axis (2..1024, at most 2^28 in all): n, or nx,ny,nz")
    ap.add_argument("--level", type=float, default=0.0)
    ap.add_argument("--supports", action="store_true", help="also measure the support mask of support_solid for --up and --r2")
    ap.add_argument("--up", default="+z", choices=UPS, help="the build direction of --supports")
    ap.add_argument("--r2", type=int, default=1, help="the squared reach of --supports (index units, 0..255)")
    ap.add_argument("--fail-on", default="", help='e.g. "area>40,contact>0.5": exit status 2 when one of them holds')
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
        lo, hi, shape = _three(a.lo, float, "--lo"), _three(a.hi, float, "--hi"), _three(a.res, int, "--res")
        report, step = solid_report(res, lo, hi, shape, a.level)
        if a.supports:
            report.update(supports_report(res, lo, hi, shape, a.level, a.up, a.r2, step))
    finally:
        res.close()
    values = {k: report[k] for k in GATES if k in report and not math.isnan(report[k])}
    report["failed"] = failed_gates(gates, values)
    for k in ("area", "contact_area"):
        if k in report:
            report[k] = _json_number(report[k])
    print(json.dumps(report))
    return 2 if report["failed"] else 0


if __name__ == "__main__":
    sys.exit(main())
