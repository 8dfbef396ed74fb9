"""Triangle meshes from RayMarchingResources.extract_mesh, and their files: Wavefront OBJ, binary little-endian PLY (with
normals, and vertex colours from a material table) and binary STL.

  python -m ray_marching_amd.mesh --scene g32 --lo -2.5 --hi 2.5 --res 256 out.ply
  python -m ray_marching_amd.mesh --scene g32 --lo -2.5 --hi 2.5 --res 1024 --sparse out.ply

extracts the surface of a named scene (csg.scene) on the GPU and writes it; the format follows the file's extension.
Triangles are wound counter-clockwise seen from outside.  The mesh is open where the surface leaves the box [lo, hi].
read() reads the three formats back (and ASCII STL and ASCII PLY): the source of RayMarchingResources.voxelize_mesh."""
import argparse
import struct
import sys

import numpy as np


def _numpy(a):
    if a is None or isinstance(a, np.ndarray):
        return a
    return a.cpu().numpy()     # a torch tensor (device=True)


class Mesh:
    """vertices (V, 3) float32; triangles (T, 3) vertex indices (uint32; int32 views as torch tensors); per vertex,
    when extracted: normals (V, 3), leaf and material (V,) (rm_query_points at the vertex positions), else None.
    stats: the statistics of a sparse extraction (a dict: vertices, triangles, bricks, bricks_kept, evaluations,
    scratch_bytes), else None."""
    stats = None

    def __init__(self, vertices, triangles, normals=None, leaf=None, material=None):
        self.vertices, self.triangles, self.normals, self.leaf, self.material = vertices, triangles, normals, leaf, material

    def __repr__(self):
        return "Mesh(%d vertices, %d triangles)" % (len(self.vertices), len(self.triangles))

    def numpy(self):
        """This mesh with numpy arrays (triangles as uint32)."""
        t = _numpy(self.triangles)
        m = Mesh(_numpy(self.vertices), t.view(np.uint32) if t.dtype == np.int32 else t, _numpy(self.normals),
                 _numpy(self.leaf), _numpy(self.material))
        m.stats = self.stats
        return m

    def is_closed(self):
        """Whether every directed edge (u, v) of the triangles occurs as often as (v, u): no border, consistent winding."""
        t = self.numpy().triangles.astype(np.int64)
        if len(t) == 0:
            return True
        u = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
        v = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
        n = int(t.max()) + 1
        fwd, nf = np.unique(u * n + v, return_counts=True)
        rev, nr = np.unique(v * n + u, return_counts=True)
        return bool(np.array_equal(fwd, rev) and np.array_equal(nf, nr))


def weld(mesh):
    """The mesh with vertices of identical binary32 coordinates (-0 folded into +0) united and the triangles re-indexed: what a
    soup (read_stl) needs before RayMarchingResources.slice_mesh, which pairs edges by vertex index.  On the host.  A vertex keeps
    the place of its first occurrence; a NaN coordinate unites only with the same bit pattern; per-vertex attributes are dropped
    (the united vertices need not agree on them)."""
    m = mesh.numpy()
    v = np.ascontiguousarray(np.asarray(m.vertices, dtype=np.float32).reshape(-1, 3)) + np.float32(0.0)   # (-0 + 0 = +0)
    if len(v) == 0:
        return Mesh(v, np.asarray(m.triangles).astype(np.uint32).reshape(-1, 3))
    bits = v.view(np.uint32).reshape(-1, 3)
    _, first, inverse = np.unique(bits, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                 # the united vertices by first occurrence
    place = np.empty(len(order), dtype=np.int64)
    place[order] = np.arange(len(order))
    t = np.asarray(m.triangles).astype(np.int64).reshape(-1, 3)
    inside = t < len(v)
    new = np.where(inside, place[inverse.reshape(-1)][np.where(inside, t, 0)], 0xFFFFFFFF)      # (an index out of range stays out of range)
    return Mesh(v[first[order]], new.astype(np.uint32))


def write_obj(mesh, path):
    """Wavefront OBJ: v, vn (when the mesh has normals) and f lines, 1-based."""
    m = mesh.numpy()
    with open(path, "w") as f:
        f.write("# %d vertices, %d triangles\n" % (len(m.vertices), len(m.triangles)))
        f.writelines("v %.9g %.9g %.9g\n" % tuple(v) for v in m.vertices.tolist())
        t = m.triangles.astype(np.int64) + 1
        if m.normals is not None:
            f.writelines("vn %.9g %.9g %.9g\n" % tuple(n) for n in m.normals.tolist())
            f.writelines("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in t.tolist())
        else:
            f.writelines("f %d %d %d\n" % tuple(x) for x in t.tolist())


def write_ply(mesh, path, materials=None):
    """Binary little-endian PLY: float x y z, nx ny nz (when the mesh has normals), uchar red green blue (from
    materials[material], rgb in [0, 1], when a table is given and the mesh has materials); faces as uchar count + 3 uint."""
    m = mesh.numpy()
    V = len(m.vertices)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if m.normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    colours = materials is not None and m.material is not None
    if colours:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    v = np.empty(V, dtype=fields)
    v["x"], v["y"], v["z"] = m.vertices[:, 0], m.vertices[:, 1], m.vertices[:, 2]
    if m.normals is not None:
        v["nx"], v["ny"], v["nz"] = m.normals[:, 0], m.normals[:, 1], m.normals[:, 2]
    if colours:
        table = np.clip(np.rint(np.asarray(materials, dtype=np.float64)[:, :3] * 255.0), 0, 255).astype(np.uint8)
        rgb = table[np.minimum(m.material.astype(np.int64), len(table) - 1)]
        v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    f = np.empty(len(m.triangles), dtype=[("n", "u1"), ("v", "<u4", (3,))])
    f["n"] = 3
    f["v"] = m.triangles
    kinds = {"<f4": "float", "u1": "uchar"}
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % V]
    head += ["property %s %s" % (kinds[t], n) for n, t in fields]
    head += ["element face %d" % len(f), "property list uchar uint vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(head) + "\n").encode("ascii"))
        out.write(v.tobytes())
        out.write(f.tobytes())


def facet_normals(vertices, triangles):
    """Unit normal of each triangle from its vertices ((b - a) x (c - a), float32; zero for a degenerate one)."""
    p = np.asarray(vertices, dtype=np.float32)[np.asarray(triangles, dtype=np.int64)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).astype(np.float32)
    length = np.sqrt((n * n).sum(axis=1, dtype=np.float32))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(length[:, None] > 0, n / length[:, None], np.float32(0)).astype(np.float32)


def write_stl(mesh, path):
    """Binary STL: 80-byte header, triangle count, then per triangle a float32 facet normal, three vertices and a zero
    attribute word."""
    m = mesh.numpy()
    rec = np.zeros(len(m.triangles), dtype=[("n", "<f4", (3,)), ("v", "<f4", (3, 3)), ("attr", "<u2")])
    rec["n"] = facet_normals(m.vertices, m.triangles)
    rec["v"] = m.vertices[m.triangles.astype(np.int64)]
    with open(path, "wb") as out:
        out.write(b"ray-marching_amd mesh export".ljust(80, b" "))
        out.write(struct.pack("<I", len(rec)))
        out.write(rec.tobytes())


def write(mesh, path, materials=None):
    """write_obj / write_ply / write_stl by the extension of `path`."""
    ext = path.lower().rsplit(".", 1)[-1]
    if ext == "obj":
        write_obj(mesh, path)
    elif ext == "ply":
        write_ply(mesh, path, materials)
    elif ext == "stl":
        write_stl(mesh, path)
    else:
        raise ValueError("unknown mesh format .%s (obj, ply or stl)" % ext)


def read_obj(path):
    """Wavefront OBJ: the v and f lines; a polygon is fanned from its first corner, a corner's index is what stands before its
    first slash, 1-based or negative (counted back from the vertices read so far)."""
    verts, tris = [], []
    with open(path) as f:
        for line in f:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                verts.append((float(p[1]), float(p[2]), float(p[3])))
            elif p[0] == "f":
                idx = []
                for corner in p[1:]:
                    k = int(corner.split("/")[0])
                    k = k - 1 if k > 0 else len(verts) + k
                    if k < 0 or k >= len(verts):
                        raise ValueError("%s: face corner %r names no vertex read so far" % (path, corner))
                    idx.append(k)
                if len(idx) < 3:
                    raise ValueError("%s: a face of %d corners" % (path, len(idx)))
                tris += [(idx[0], idx[m], idx[m + 1]) for m in range(1, len(idx) - 1)]
    return Mesh(np.array(verts, dtype=np.float32).reshape(-1, 3), np.array(tris, dtype=np.uint32).reshape(-1, 3))


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path):
    """PLY, ASCII or binary little-endian: the vertex element's x, y, z (and nx, ny, nz when all three are there) and the face
    element's index list, polygons fanned; other properties and elements are skipped."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("%s is not a PLY file" % path)
    body = data.index(b"\n", end) + 1
    fmt, elements = None, []                                     # elements: [name, count, [(kind, name, type[, count type])]]
    for line in data[:end].decode("ascii").splitlines():
        p = line.split()
        if not p:
            continue
        if p[0] == "format":
            fmt = p[1]
        elif p[0] == "element":
            elements.append([p[1], int(p[2]), []])
        elif p[0] == "property":
            if p[1] == "list":
                elements[-1][2].append(("list", p[4], _PLY_TYPES[p[3]], _PLY_TYPES[p[2]]))
            else:
                elements[-1][2].append(("scalar", p[2], _PLY_TYPES[p[1]]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError("%s: PLY format %r (ascii or binary_little_endian)" % (path, fmt))
    verts = normals = None
    tris = []
    tokens = iter(data[body:].split()) if fmt == "ascii" else None
    pos = body
    for name, count, props in elements:
        scalar_only = all(p[0] == "scalar" for p in props)
        if scalar_only:
            dt = np.dtype([(p[1], "<" + p[2]) for p in props])
            if fmt == "ascii":
                rows = np.array([tuple(float(next(tokens)) for _ in props) for _ in range(count)], dtype=np.float64).reshape(count, len(props))
                table = {p[1]: rows[:, k] for k, p in enumerate(props)}
            else:
                rec = np.frombuffer(data, dtype=dt, count=count, offset=pos)
                pos += dt.itemsize * count
                table = {p[1]: rec[p[1]] for p in props}
            if name == "vertex":
                verts = np.stack([table["x"], table["y"], table["z"]], axis=1).astype(np.float32)
                if all(k in table for k in ("nx", "ny", "nz")):
                    normals = np.stack([table["nx"], table["ny"], table["nz"]], axis=1).astype(np.float32)
            continue
        if fmt != "ascii" and len(props) == 1 and name == "face" and count:     # all triangles (what write_ply writes): at once
            dt = np.dtype([("n", "<" + props[0][3]), ("v", "<" + props[0][2], (3,))])
            if pos + dt.itemsize * count <= len(data):
                rec = np.frombuffer(data, dtype=dt, count=count, offset=pos)
                if np.all(rec["n"] == 3):
                    tris += rec["v"].tolist()
                    pos += dt.itemsize * count
                    continue
        for _ in range(count):                                   # an element with lists: row by row
            for p in props:
                if p[0] == "scalar":
                    if fmt == "ascii":
                        next(tokens)
                    else:
                        pos += np.dtype(p[2]).itemsize
                    continue
                if fmt == "ascii":
                    n = int(next(tokens))
                    idx = [int(next(tokens)) for _ in range(n)]
                else:
                    n = int(np.frombuffer(data, dtype="<" + p[3], count=1, offset=pos)[0])
                    pos += np.dtype(p[3]).itemsize
                    idx = np.frombuffer(data, dtype="<" + p[2], count=n, offset=pos).tolist()
                    pos += np.dtype(p[2]).itemsize * n
                if name == "face" and p[1] in ("vertex_indices", "vertex_index"):
                    tris += [(idx[0], idx[m], idx[m + 1]) for m in range(1, n - 1)]
    if verts is None:
        raise ValueError("%s has no vertex element" % path)
    return Mesh(verts, np.array(tris, dtype=np.uint32).reshape(-1, 3), normals)


def read_stl(path):
    """STL, binary or ASCII: a soup -- three vertices per triangle in file order, not welded; triangles (T, 3) = 0 .. 3 T - 1."""
    with open(path, "rb") as f:
        data = f.read()
    n = struct.unpack_from("<I", data, 80)[0] if len(data) >= 84 else None
    if n is not None and len(data) == 84 + 50 * n:               # (a binary file may begin with "solid", too: the size decides)
        rec = np.frombuffer(data, dtype=[("n", "<f4", (3,)), ("v", "<f4", (3, 3)), ("attr", "<u2")], count=n, offset=84)
        verts = np.ascontiguousarray(rec["v"].reshape(-1, 3))
    else:
        text = data.decode("ascii", errors="replace").split()
        if not text or text[0] != "solid":
            raise ValueError("%s is neither a binary nor an ASCII STL file" % path)
        coords = [float(text[k + 1 + m]) for k, w in enumerate(text) if w == "vertex" for m in range(3)]
        verts = np.array(coords, dtype=np.float32).reshape(-1, 3)
        if len(verts) % 3:
            raise ValueError("%s: %d vertices are not whole triangles" % (path, len(verts)))
    return Mesh(verts, np.arange(len(verts), dtype=np.uint32).reshape(-1, 3))


def read(path):
    """read_obj / read_ply / read_stl by the extension of `path`: what write() writes, and the ASCII forms of PLY and STL."""
    ext = path.lower().rsplit(".", 1)[-1]
    if ext == "obj":
        return read_obj(path)
    if ext == "ply":
        return read_ply(path)
    if ext == "stl":
        return read_stl(path)
    raise ValueError("unknown mesh format .%s (obj, ply or stl)" % ext)


# The albedo table the CLI uploads to its context before extracting, so a PLY's colours are those the context's draws show.
# Untagged surfaces render in (0.4, 0.7, 0.1) whatever the table holds (wgsl:105), and entry 0 is that colour, so an
# untagged scene (every vertex material 0) comes out in the one colour it renders in.  The material scenes of the tests use the same table (tests/scenes.py MATERIAL_TABLE;
# tests/test_mesh_cpu.py checks that the two agree).
MATERIALS = [(0.4, 0.7, 0.1), (0.9, 0.15, 0.1), (0.1, 0.3, 0.9), (0.95, 0.9, 0.2), (0.8, 0.8, 0.8), (0.6, 0.1, 0.7)]


def _three(text, kind, name):
    """'v' or 'x,y,z' -> three values."""
    try:
        v = [kind(x) for x in text.split(",")]
    except ValueError:
        raise SystemExit("%s: %r is not a number or a comma-separated triple" % (name, text))
    if len(v) not in (1, 3):
        raise SystemExit("%s takes 1 or 3 comma-separated values, not %r" % (name, text))
    return v * 3 if len(v) == 1 else v


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ray_marching_amd.mesh", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="g32", help="a csg.scene name (g1, g8, g32, g32_balanced, mat_mix, ...)")
    ap.add_argument("--lo", default="-3", help="lower box corner: one value for all axes, or x,y,z")
    ap.add_argument("--hi", default="3", help="upper box corner: one value, or x,y,z")
    ap.add_argument("--res", default="128", help="lattice points per axis: n, or nx,ny,nz")
    ap.add_argument("--level", type=float, default=0.0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-normals", action="store_true")
    ap.add_argument("--sparse", action="store_true",
                    help="extract brick by brick (rm_extract_mesh_sparse): the same mesh, any lattice size; prints its statistics")
    ap.add_argument("out", help="output file: .obj, .ply or .stl")
    a = ap.parse_args(argv)
    from . import csg, renderer
    res = renderer.RayMarchingResources(a.device)
    try:
        res.set_materials(MATERIALS)
        res.set_scene(csg.scene(a.scene))
        extract = res.extract_mesh_sparse if a.sparse else res.extract_mesh
        m = extract(_three(a.lo, float, "--lo"), _three(a.hi, float, "--hi"), _three(a.res, int, "--res"), level=a.level,
                    normals=not a.no_normals, ids=True)
    finally:
        res.close()
    write(m, a.out, MATERIALS)
    print("%s: %d vertices, %d triangles, %s" % (a.out, len(m.vertices), len(m.triangles),
                                                 "closed" if m.is_closed() else "open (the surface meets the box)"))
    if a.sparse:
        print("sparse: %d of %d bricks kept, %d evaluations, %.1f MB of scratch"
              % (m.stats["bricks_kept"], m.stats["bricks"], m.stats["evaluations"], m.stats["scratch_bytes"] / 1e6))


if __name__ == "__main__":
    sys.exit(main())
