"""Slices from RayMarchingResources.slice_contours -- the outlines of the solid in a stack of parallel planes, as ordered
polylines -- and their files: SVG (section drawings) and an ASCII layer file in the style of the Common Layer Interface.

  python -m ray_marching_amd.slicer --scene g8 --axis y --lo -2 --hi 2 --res 1024 --layer-height 0.05 out.svg

slices a named scene (csg.scene) on the GPU and writes the layers; the format follows the file's extension (.svg, .cli).

  python -m ray_marching_amd.slicer --mesh part.stl --axis z --layer-height 0.2 out.svg

slices a mesh file (mesh.read: STL, OBJ, PLY; welded first) instead, prints its counts as one JSON object, and with
--fail-on "open_contours>0,branch_edges>0,border_edges>0" exits with status 2 when a gate trips.
With --hatch SPACING (and --hatch-angle, --hatch-rotate, --zigzag) either kind of run also fills every layer with parallel lines
(RayMarchingResources.hatch_slices), writes them into the file, prints the hatch counts as JSON (`segments` as `hatch_segments`)
and lets --fail-on name them, e.g. "odd_lines>0".
Seen from the positive end of the slicing axis, outer boundaries run counter-clockwise and holes clockwise.  A contour is
open where the outline leaves the box [lo, hi]."""
import argparse
import sys

import numpy as np


def _numpy(a):
    if a is None or isinstance(a, np.ndarray):
        return a
    return a.cpu().numpy()     # a torch tensor (device=True)


def _unsigned(a):
    return a.view(np.uint32) if a is not None and a.dtype == np.int32 else a


class Slices:
    """points (P, 3) float32, world x, y, z in contour order; contours (C, 4) (first point, point count, layer, closed 0/1);
    layer_first (n_layers + 1,): the contour each layer starts at, the last entry is C (uint32; int32 views as torch
    tensors); heights (n_layers,) float32 as given to the call; axis: the slicing axis w (0, 1, 2) -- the in-plane axes are
    u = (w + 1) % 3 and v = (w + 2) % 3; per point, when computed: normals (P, 3), leaf and material (P,) (rm_query_points
    at the points), else None.  lattice: (origin_uv, step_uv, (nu, nv)) of the layers, or None."""

    counts = stats = None     # of a mesh slicing (RayMarchingResources.slice_mesh): dicts, else None

    def __init__(self, points, contours, layer_first, heights, axis, normals=None, leaf=None, material=None, lattice=None):
        self.points, self.contours, self.layer_first = points, contours, layer_first
        self.heights, self.axis = np.asarray(heights, dtype=np.float32), int(axis)
        self.normals, self.leaf, self.material, self.lattice = normals, leaf, material, lattice

    def __repr__(self):
        return "Slices(%d layers, %d contours, %d points)" % (len(self.heights), len(self.contours), len(self.points))

    def numpy(self):
        """These slices with numpy arrays (contours and layer_first as uint32)."""
        s = Slices(_numpy(self.points), _unsigned(_numpy(self.contours)), _unsigned(_numpy(self.layer_first)), self.heights,
                   self.axis, _numpy(self.normals), _unsigned(_numpy(self.leaf)), _unsigned(_numpy(self.material)), self.lattice)
        s.counts, s.stats = self.counts, self.stats
        return s

    @property
    def in_plane_axes(self):
        return (self.axis + 1) % 3, (self.axis + 2) % 3

    def contour(self, c):
        """((n, 2) float32 in-plane points (u, v) in order, closed).  A closed contour does not repeat its first point."""
        s = self.numpy()
        first, count, _, closed = (int(x) for x in s.contours[c])
        return s.points[first:first + count][:, list(self.in_plane_axes)], bool(closed)

    def layer(self, k):
        """The contours of layer k, in order: a list of ((n, 2) points, closed)."""
        s = self.numpy()
        return [s.contour(c) for c in range(int(s.layer_first[k]), int(s.layer_first[k + 1]))]

    def area(self, k):
        """The area of layer k's solid: the float64 shoelace sum over its closed contours (holes run clockwise and subtract)."""
        total = 0.0
        for uv, closed in self.layer(k):
            if closed:
                total += shoelace(uv)
        return total


class Hatch:
    """The hatch of slices (RayMarchingResources.hatch_slices): segments (H, 4) float32, in-plane (u, v) of the first end and of the
    second; line (H,): layer * n_lines + j of each segment; layer_first (n_layers + 1,): the segment each layer starts at, the last
    entry is H (uint32; int32 views as torch tensors); lines (n_layers, 4) float32 (dx, dy, offset, spacing) and n_lines as given
    to the call; counts and stats: dicts (_ffi.HATCH_COUNT_NAMES, HATCH_STAT_NAMES)."""

    def __init__(self, segments, line, layer_first, lines, n_lines, counts=None, stats=None):
        self.segments, self.line, self.layer_first = segments, line, layer_first
        self.lines, self.n_lines, self.counts, self.stats = np.asarray(lines, dtype=np.float32), int(n_lines), counts, stats

    def __repr__(self):
        return "Hatch(%d layers, %d segments)" % (len(self.lines), len(self.segments))

    def numpy(self):
        """This hatch with numpy arrays (line and layer_first as uint32)."""
        return Hatch(_numpy(self.segments), _unsigned(_numpy(self.line)), _unsigned(_numpy(self.layer_first)), self.lines, self.n_lines,
                     self.counts, self.stats)

    def layer(self, k):
        """The segments of layer k, in order: (m, 4) float32."""
        h = self.numpy()
        return h.segments[int(h.layer_first[k]):int(h.layer_first[k + 1])]

    def length(self, k):
        """The total length of layer k's segments, float64, on the host."""
        g = self.layer(k).astype(np.float64)
        return float(np.sum(np.hypot(g[:, 2] - g[:, 0], g[:, 3] - g[:, 1])))


def hatch_lines(slices, spacing, angle=45.0, rotate=90.0):
    """(lines, n_lines) for RayMarchingResources.hatch_slices: layer k is hatched along the angle (angle + k * rotate) % 360 degrees,
    counter-clockwise from +u, with lines `spacing` apart.  lines: (n_layers, 4) float32 (dx, dy, offset, spacing); the direction
    is d = (float32 cos, float32 sin) -- a unit vector only to binary32 rounding (its length is within 2^-23 of 1), which is all
    the contract asks: offset and spacing are in units of s = v dx - u dy.  Lines are anchored at the world origin, at
    s = (j + 0.5) * spacing for integer j, so that layers of one direction register whatever their outline: offset =
    (j0 + 0.5) * spacing with j0 = floor(s_min / spacing) - 1 and s_min the smallest s over the four corners of the slices' in-plane
    extent (the lattice, or the points' bounding box).  One n_lines serves all layers, large enough for the widest: every point's s
    lies strictly inside (c_0, c_{n_lines - 1}).  The angle is reduced modulo 360 before its cosine is taken, so with rotate = 90
    layers k and k + 4 get the same bits; layers k and k + 2 run along opposite directions, which are the same set of lines only
    as far as cos and sin of t and t + 180 degrees negate each other exactly."""
    sp = np.float32(spacing)
    if not (np.isfinite(sp) and sp > 0):
        raise ValueError("spacing %r must be finite and > 0" % (spacing,))
    u0, v0, u1, v1 = _extent(slices.numpy())
    n_layers = len(slices.heights)
    lines = np.zeros((n_layers, 4), dtype=np.float32)
    n_lines = 1
    for k in range(n_layers):
        theta = np.radians((float(angle) + k * float(rotate)) % 360.0)
        dx, dy = np.float32(np.cos(theta)), np.float32(np.sin(theta))
        s = [v * float(dx) - u * float(dy) for u in (u0, u1) for v in (v0, v1)]
        j0 = np.floor(min(s) / float(sp)) - 1.0
        off = np.float32((j0 + 0.5) * float(sp))
        n = int(np.ceil((max(s) - float(off)) / float(sp))) + 2
        while float(off) + (n - 1) * float(sp) <= max(s):      # (a rounded offset far from the origin)
            n += 1
        lines[k] = (dx, dy, off, sp)
        n_lines = max(n_lines, n)
    if n_lines > 1 << 24:
        raise ValueError("spacing %g gives %d lines per layer: at most 2^24" % (float(sp), n_lines))
    return lines, n_lines


def _hatch_of(hatch, slices):
    """The hatch as numpy, checked against the slices it goes with; None for None."""
    if hatch is None:
        return None
    h = hatch.numpy()
    if len(h.layer_first) != len(slices.heights) + 1:
        raise ValueError("the hatch has %d layers, the slices %d" % (len(h.layer_first) - 1, len(slices.heights)))
    return h


def shoelace(uv):
    """Signed area of the closed polygon through (n, 2) points, float64: positive for counter-clockwise."""
    p = np.asarray(uv, dtype=np.float64)
    x, y = p[:, 0], p[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def _extent(s):
    """(u0, v0, u1, v1): the layers' lattice, or the bounding box of the points when the slices carry none."""
    if s.lattice is not None:
        (ou, ov), (su, sv), (nu, nv) = s.lattice
        return float(ou), float(ov), float(ou) + (nu - 1) * float(su), float(ov) + (nv - 1) * float(sv)
    if len(s.points) == 0:
        return 0.0, 0.0, 1.0, 1.0
    uv = s.points[:, list(s.in_plane_axes)].astype(np.float64)
    return float(uv[:, 0].min()), float(uv[:, 1].min()), float(uv[:, 0].max()), float(uv[:, 1].max())


def write_svg(slices, path, hatch=None):
    """SVG: one <g id="layer-k" data-height="..."> per layer holding one <path fill-rule="evenodd"> with all the layer's
    contours -- "M u v L u v ... Z" for a closed one, without the Z for an open one --, inside one <g> that flips v so the
    drawing is seen from the positive end of the slicing axis.  The viewBox is the layers' lattice.  Coordinates are
    written with %.9g: every float32 round-trips.  With a `hatch` (a Hatch of these slices) every layer's group also holds its
    hatch segments as one unfilled <path>, "M u v L u v" each."""
    s = slices.numpy()
    fill = _hatch_of(hatch, s)
    u0, v0, u1, v1 = _extent(s)
    w, h = max(u1 - u0, 1e-30), max(v1 - v0, 1e-30)
    stroke = 0.002 * max(w, h)
    with open(path, "w") as f:
        f.write('<?xml version="1.0" encoding="UTF-8"?>\n')
        f.write('<svg xmlns="http://www.w3.org/2000/svg" viewBox="%.9g %.9g %.9g %.9g">\n' % (u0, -v1, w, h))
        f.write('<g transform="scale(1,-1)" fill="#9aba4a" fill-opacity="0.25" stroke="#203000" stroke-width="%.9g">\n' % stroke)
        for k in range(len(s.heights)):
            f.write('<g id="layer-%d" data-height="%.9g">\n' % (k, s.heights[k]))
            d = []
            for uv, closed in s.layer(k):
                pts = uv.tolist()
                d.append("M %.9g %.9g" % tuple(pts[0]) + "".join(" L %.9g %.9g" % tuple(p) for p in pts[1:]) + (" Z" if closed else ""))
            if d:
                f.write('<path fill-rule="evenodd" d="%s"/>\n' % " ".join(d))
            if fill is not None and len(fill.layer(k)):
                f.write('<path fill="none" d="%s"/>\n' % " ".join("M %.9g %.9g L %.9g %.9g" % tuple(g) for g in fill.layer(k).tolist()))
            f.write("</g>\n")
        f.write("</g>\n</svg>\n")


def write_cli(slices, path, hatch=None):
    """An ASCII layer file in the style of the Common Layer Interface.  Exactly this is written: the header lines
    $$HEADERSTART, $$ASCII, $$UNITS/1, $$VERSION/200, $$LABEL/1,ray-marching_amd, $$LAYERS/<number of layers>, $$HEADEREND;
    then $$GEOMETRYSTART, per layer "$$LAYER/<height>" followed by one "$$POLYLINE/1,<dir>,<n>,u1,v1,...,un,vn" per contour,
    and $$GEOMETRYEND.  dir is 1 for a counter-clockwise contour, 0 for a clockwise one and 2 for an open one; a closed
    polyline repeats its first point as its last (n counts it); coordinates are in-plane (u, v), written with %.9g.  No
    specification of the format was at hand: the file is unverified against a third-party reader.  With a `hatch` (a Hatch of
    these slices) every layer that has hatch segments also gets one "$$HATCHES/1,<n>,u,v,u,v,..." record after its polylines: n
    segments, the first end and the second of each."""
    s = slices.numpy()
    fill = _hatch_of(hatch, s)
    with open(path, "w") as f:
        f.write("$$HEADERSTART\n$$ASCII\n$$UNITS/1\n$$VERSION/200\n$$LABEL/1,ray-marching_amd\n$$LAYERS/%d\n$$HEADEREND\n" % len(s.heights))
        f.write("$$GEOMETRYSTART\n")
        for k in range(len(s.heights)):
            f.write("$$LAYER/%.9g\n" % s.heights[k])
            for uv, closed in s.layer(k):
                direction = (1 if shoelace(uv) > 0 else 0) if closed else 2
                pts = uv.tolist() + ([uv[0].tolist()] if closed else [])
                f.write("$$POLYLINE/1,%d,%d,%s\n" % (direction, len(pts), ",".join("%.9g,%.9g" % tuple(p) for p in pts)))
            if fill is not None and len(fill.layer(k)):
                f.write("$$HATCHES/1,%d,%s\n" % (len(fill.layer(k)), ",".join("%.9g,%.9g,%.9g,%.9g" % tuple(g) for g in fill.layer(k).tolist())))
        f.write("$$GEOMETRYEND\n")


def write(slices, path, hatch=None):
    """write_svg / write_cli by the extension of `path`."""
    ext = path.lower().rsplit(".", 1)[-1]
    if ext == "svg":
        write_svg(slices, path, hatch)
    elif ext == "cli":
        write_cli(slices, path, hatch)
    else:
        raise ValueError("unknown slice format .%s (svg or cli)" % ext)


def _values(text, kind, name, counts):
    """'v' or comma-separated values -> a list of one of the lengths in `counts` (a single value is repeated)."""
    try:
        v = [kind(x) for x in text.split(",")]
    except ValueError:
        raise SystemExit("%s: %r is not a number or a comma-separated list" % (name, text))
    if len(v) == 1:
        return v * max(counts)
    if len(v) not in counts:
        raise SystemExit("%s takes %s comma-separated values, not %r" % (name, " or ".join(str(c) for c in (1,) + tuple(counts)), text))
    return v


_GATE_OPS = {">=": lambda a, b: a >= b, "<=": lambda a, b: a <= b, "==": lambda a, b: a == b, "!=": lambda a, b: a != b,
             ">": lambda a, b: a > b, "<": lambda a, b: a < b}


def parse_gates(text, names):
    """'open_contours>0,branch_edges>0' -> [(name, op, value)]; names: the counts a gate may test."""
    gates = []
    for term in (t.strip() for t in text.split(",") if t.strip()):
        for op in (">=", "<=", "==", "!=", ">", "<"):
            if op in term:
                name, value = (x.strip() for x in term.split(op, 1))
                break
        else:
            raise SystemExit("--fail-on: %r has no comparison (>, >=, <, <=, ==, !=)" % term)
        if name not in names:
            raise SystemExit("--fail-on: %r is not one of %s" % (name, ", ".join(names)))
        try:
            gates.append((name, op, int(value)))
        except ValueError:
            raise SystemExit("--fail-on: %r is not an integer" % value)
    return gates


def tripped_gates(gates, counts):
    """The gates of parse_gates that hold for `counts`, as text."""
    return ["%s%s%d" % (n, op, v) for n, op, v in gates if _GATE_OPS[op](int(counts[n]), v)]


def hatch_count_keys(counts):
    """The hatch counts under the names the command line prints and gates them by: their own, except that `segments` -- a name
    the mesh slicing's counts have too -- becomes `hatch_segments`."""
    return {("hatch_segments" if n == "segments" else n): v for n, v in counts.items()}


def _check_hatch_arguments(a):
    if a.hatch is None:
        if a.zigzag or a.hatch_angle is not None or a.hatch_rotate is not None:
            raise SystemExit("--hatch-angle, --hatch-rotate and --zigzag go with --hatch SPACING")
    elif not (np.isfinite(a.hatch) and a.hatch > 0):
        raise SystemExit("--hatch: the spacing %r must be a finite number > 0" % a.hatch)


def _hatch(res, a, s):
    """The Hatch the command line asks for (None without --hatch), while the context still holds the slices `s`."""
    if a.hatch is None:
        return None
    lines, n_lines = hatch_lines(s, a.hatch, 45.0 if a.hatch_angle is None else a.hatch_angle, 90.0 if a.hatch_rotate is None else a.hatch_rotate)
    return res.hatch_slices(lines, n_lines, zigzag=a.zigzag)


def _main_mesh(a):
    import json
    from . import _ffi, mesh as _mesh, renderer
    names = _ffi.MSLICE_COUNT_NAMES + (tuple(hatch_count_keys(dict.fromkeys(_ffi.HATCH_COUNT_NAMES))) if a.hatch is not None else ())
    gates = parse_gates(a.fail_on, names) if a.fail_on else []
    if a.layer_height is None:
        raise SystemExit("--mesh needs --layer-height")
    m = _mesh.weld(_mesh.read(a.mesh))
    res = renderer.RayMarchingResources(a.device)
    try:
        s = res.slice_mesh_box(m, axis=a.axis, layer_height=a.layer_height, resolution=int(_values(a.res, int, "--res", (2,))[0]))
        h = _hatch(res, a, s)
    finally:
        res.close()
    write(s, a.out, h)
    counts = dict(s.counts, **(hatch_count_keys(h.counts) if h is not None else {}))
    print(json.dumps(dict(counts, layers=len(s.heights), out=a.out)))
    bad = tripped_gates(gates, counts)
    if bad:
        print("gate tripped: %s" % ", ".join(bad), file=sys.stderr)
        return 2
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ray_marching_amd.slicer", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32", help="a csg.scene name (g1, g8, g32, g32_balanced, mat_mix, ...)")
    ap.add_argument("--mesh", default=None, help="slice this mesh file (.stl, .obj, .ply) instead of a scene; takes --axis, --layer-height, --res")
    ap.add_argument("--fail-on", default=None, help='with --mesh: gates on the counts, e.g. "open_contours>0,branch_edges>0,border_edges>0"; exit 2 when one trips')
    ap.add_argument("--axis", default="y", help="the slicing axis: x, y or z (default y: the floor's up axis)")
    ap.add_argument("--lo", default="-3", help="lower box corner: one value for all axes, or x,y,z")
    ap.add_argument("--hi", default="3", help="upper box corner: one value, or x,y,z")
    ap.add_argument("--res", default="1024", help="lattice points per in-plane axis: n, or nu,nv")
    ap.add_argument("--layer-height", type=float, default=None, help="slice mid-layer every this much from lo to hi on the axis")
    ap.add_argument("--heights", default=None, help="comma-separated heights on the axis, instead of --layer-height")
    ap.add_argument("--level", type=float, default=0.0)
    ap.add_argument("--hatch", type=float, default=None, metavar="SPACING", help="fill every layer with parallel lines this far apart (even-odd rule)")
    ap.add_argument("--hatch-angle", type=float, default=None, help="with --hatch: the first layer's direction in degrees from +u (default 45)")
    ap.add_argument("--hatch-rotate", type=float, default=None, help="with --hatch: the change of direction from layer to layer, degrees (default 90)")
    ap.add_argument("--zigzag", action="store_true", help="with --hatch: every other line runs backwards")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("out", help="output file: .svg or .cli")
    a = ap.parse_args(argv)
    if a.axis not in ("x", "y", "z"):
        raise SystemExit("--axis takes x, y or z, not %r" % a.axis)
    _check_hatch_arguments(a)
    if a.mesh is not None:
        return _main_mesh(a)
    if a.fail_on is not None and a.hatch is None:
        raise SystemExit("--fail-on goes with --mesh or --hatch")
    if (a.heights is None) == (a.layer_height is None):
        raise SystemExit("give either --layer-height or --heights")
    heights = None
    if a.heights is not None:
        try:
            heights = [float(x) for x in a.heights.split(",")]
        except ValueError:
            raise SystemExit("--heights: %r is not a comma-separated list of numbers" % a.heights)
    from . import _ffi, csg, renderer
    gates = parse_gates(a.fail_on, tuple(hatch_count_keys(dict.fromkeys(_ffi.HATCH_COUNT_NAMES)))) if a.fail_on else []
    res = renderer.RayMarchingResources(a.device)
    try:
        res.set_scene(csg.scene(a.scene))
        s = res.slice_contours(_values(a.lo, float, "--lo", (3,)), _values(a.hi, float, "--hi", (3,)), _values(a.res, int, "--res", (2,)),
                               heights=heights, layer_height=a.layer_height, axis=a.axis, level=a.level)
        h = _hatch(res, a, s)
    finally:
        res.close()
    write(s, a.out, h)
    closed = int(np.count_nonzero(s.contours[:, 3])) if len(s.contours) else 0
    print("%s: %d layers, %d contours (%d closed, %d open), %d points"
          % (a.out, len(s.heights), len(s.contours), closed, len(s.contours) - closed, len(s.points)))
    if h is not None:
        import json
        counts = hatch_count_keys(h.counts)
        print(json.dumps(dict(counts, layers=len(s.heights), out=a.out)))
        bad = tripped_gates(gates, counts)
        if bad:
            print("gate tripped: %s" % ", ".join(bad), file=sys.stderr)
            return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
