"""Mesh voxelisation in numpy: the contract of rm_voxelize_mesh restated twice, independently, and an exact
oracle for convex polyhedra.  Also the meshes the tests share.

  voxelize(...)          per triangle over its box of rows, vectorised int64: what the kernels do, in another order
  voxelize_by_rows(...)  per row over all triangles, Python integers, the crossings as exact fractions: a point is inside iff the
                         number of crossings with x_c <= 64 i is odd
  convex_classes(...)    strictly inside / strictly outside / on the boundary of a convex polyhedron, from the signed plane
                         determinants of the snapped vertices in Python integers

Both restatements return (occupancy uint8 (nz, ny, nx), counts: a dict of _ffi.VOX_COUNT_NAMES)."""
from fractions import Fraction

import numpy as np

FRAC = 64
MAX_Q = 1 << 17
COUNT_NAMES = ("triangles", "rejected", "edge_on", "crossings", "inside", "open_rows")


def snap(vertices, origin, step):
    """(q int64 (V, 3), valid bool (V, 3)): q = rint((double(v) - double(o)) / double(s) * 64), each operation rounded once;
    valid where the coordinate is finite and |q| <= 2^17."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    o = np.asarray(origin, dtype=np.float32).astype(np.float64)
    s = np.asarray(step, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        r = np.rint((v - o) / s * 64.0)
        valid = np.abs(r) <= MAX_Q                    # (NaN compares false)
    return np.where(valid, r, 0.0).astype(np.int64), valid


def _accepted(vertices, triangles, origin, step):
    """The snapped corners (T, 3, 3) int64 of every triangle and which are accepted; triangles None: a soup."""
    q, valid = snap(vertices, origin, step)
    nv = len(q)
    if triangles is None:
        assert nv % 3 == 0
        tri = np.arange(nv, dtype=np.int64).reshape(-1, 3)
    else:
        tri = np.asarray(triangles).astype(np.int64).reshape(-1, 3)
    in_range = (tri < nv).all(axis=1)
    safe = np.where(tri < nv, tri, 0)
    ok = in_range & valid[safe].all(axis=(1, 2))
    return q[safe], ok


def _orient(p):
    """One accepted triangle's corners (3, 3) -> (a, b, c, A2) with A2 >= 0 (b and c swapped when the projection is clockwise)."""
    a, b, c = (tuple(int(x) for x in row) for row in p)
    A2 = (b[1] - a[1]) * (c[2] - a[2]) - (b[2] - a[2]) * (c[1] - a[1])
    if A2 < 0:
        b, c, A2 = c, b, -A2
    return a, b, c, A2


def _admits(E, dy, dz):
    return E > 0 or (E == 0 and (dy > 0 or (dy == 0 and dz > 0)))


def _finish(bits, counts, shape):
    """The rows' bits (nz, ny, nx + 1) -> occupancy and the last two counts."""
    nx = shape[0]
    prefix = np.bitwise_xor.accumulate(bits.astype(np.uint8), axis=2)
    occ = np.ascontiguousarray(prefix[:, :, :nx])
    counts["inside"] = int(occ.sum())
    counts["open_rows"] = int(prefix[:, :, nx].sum())
    return occ, counts


def voxelize(vertices, triangles, origin, step, shape):
    """Per triangle over its box of rows (int64, vectorised over the box)."""
    nx, ny, nz = (int(x) for x in shape)
    P, ok = _accepted(vertices, triangles, origin, step)
    counts = dict.fromkeys(COUNT_NAMES, 0)
    counts["triangles"], counts["rejected"] = len(P), int((~ok).sum())
    bits = np.zeros((nz, ny, nx + 1), dtype=np.uint8)
    for p in P[ok]:
        a, b, c, A2 = _orient(p)
        if A2 == 0:
            counts["edge_on"] += 1
            continue
        ys, zs = (a[1], b[1], c[1]), (a[2], b[2], c[2])
        j0, j1 = max(-(-min(ys) // FRAC), 0), min(max(ys) // FRAC, ny - 1)
        k0, k1 = max(-(-min(zs) // FRAC), 0), min(max(zs) // FRAC, nz - 1)
        if j0 > j1 or k0 > k1:
            continue
        Z, Y = np.meshgrid(np.arange(k0, k1 + 1, dtype=np.int64) * FRAC, np.arange(j0, j1 + 1, dtype=np.int64) * FRAC, indexing="ij")
        admitted = np.ones(Y.shape, dtype=bool)
        E = []
        for u, v in ((b, c), (c, a), (a, b)):
            dy, dz = v[1] - u[1], v[2] - u[2]
            e = dy * (Z - u[2]) - dz * (Y - u[1])
            admitted &= (e > 0) | ((e == 0) & (dy > 0 or (dy == 0 and dz > 0)))
            E.append(e)
        num = E[0] * a[0] + E[1] * b[0] + E[2] * c[0]
        den = FRAC * A2
        t = np.clip(-((-num) // den), 0, nx)                                   # ceil(num / den)
        kk, jj = np.nonzero(admitted)
        np.bitwise_xor.at(bits, (kk + k0, jj + j0, t[kk, jj]), 1)
        counts["crossings"] += len(kk)
    return _finish(bits, counts, (nx, ny, nz))


def voxelize_by_rows(vertices, triangles, origin, step, shape):
    """Per row over all triangles: Python integers, crossings as Fractions, parity of the crossings at or before each point."""
    nx, ny, nz = (int(x) for x in shape)
    P, ok = _accepted(vertices, triangles, origin, step)
    counts = dict.fromkeys(COUNT_NAMES, 0)
    counts["triangles"], counts["rejected"] = len(P), int((~ok).sum())
    tris = []
    for p in P[ok]:
        a, b, c, A2 = _orient(p)
        if A2 == 0:
            counts["edge_on"] += 1
        else:
            tris.append((a, b, c, A2))
    occ = np.zeros((nz, ny, nx), dtype=np.uint8)
    for k in range(nz):
        Z = FRAC * k
        for j in range(ny):
            Y = FRAC * j
            xs = []
            for a, b, c, A2 in tris:
                E = []
                for u, v in ((b, c), (c, a), (a, b)):
                    dy, dz = v[1] - u[1], v[2] - u[2]
                    e = dy * (Z - u[2]) - dz * (Y - u[1])
                    if not _admits(e, dy, dz):
                        break
                    E.append(e)
                else:
                    xs.append(Fraction(E[0] * a[0] + E[1] * b[0] + E[2] * c[0], A2))
            counts["crossings"] += len(xs)
            counts["open_rows"] += len(xs) & 1
            for i in range(nx):
                occ[k, j, i] = sum(1 for x in xs if x <= FRAC * i) & 1
    counts["inside"] = int(occ.sum())
    return occ, counts


def convex_classes(vertices, triangles, origin, step, shape):
    """int8 (nz, ny, nx): +1 strictly inside, -1 strictly outside, 0 on the boundary of the convex polyhedron whose faces are the
    triangles (wound counter-clockwise seen from outside), from the snapped vertices in exact integers."""
    nx, ny, nz = (int(x) for x in shape)
    P, ok = _accepted(vertices, triangles, origin, step)
    assert ok.all()
    planes = []
    for p in P:
        a, b, c = (np.array([int(x) for x in row], dtype=object) for row in p)
        u, v = b - a, c - a
        n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
        if n != (0, 0, 0):
            planes.append((n, n[0] * a[0] + n[1] * a[1] + n[2] * a[2]))
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    X, Y, Z = (FRAC * i).astype(object), (FRAC * j).astype(object), (FRAC * k).astype(object)
    worst = None
    for n, d in planes:                                                         # signed height above each face: <= 0 inside
        h = n[0] * X + n[1] * Y + n[2] * Z - d
        worst = h if worst is None else np.maximum(worst, h)
    sign = np.sign(worst.astype(np.float64))                                    # (|h| < 2^57 is exact enough for a sign: 0 stays 0)
    return (-sign).astype(np.int8)


# ---- the meshes of the tests --------------------------------------------------------------------------------------------------
def icosphere(level, radius, centre):
    """An icosahedron subdivided `level` times (20 * 4^level triangles), wound counter-clockwise seen from outside."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = (np.array(v) * radius + np.asarray(centre, dtype=np.float64)).astype(np.float32)
    return verts, np.array(f, dtype=np.uint32)


def box(lo, hi):
    """The 12 triangles of an axis-aligned box, outward."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    v = np.array([(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)], dtype=np.float32)
    q = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (0, 4, 7, 3)]
    t = [tri for a, b, c, d in q for tri in ((a, b, c), (a, c, d))]
    return v, np.array(t, dtype=np.uint32)


def octahedron():
    v = np.array([(10, 8, 2), (10, 8, 14), (4, 8, 8), (16, 8, 8), (10, 2, 8), (10, 14, 8)], dtype=np.float32)
    # bottom 0, top 1, -x 2, +x 3, -y 4, +y 5
    t = [(1, 3, 5), (1, 5, 2), (1, 2, 4), (1, 4, 3), (0, 5, 3), (0, 2, 5), (0, 4, 2), (0, 3, 4)]
    return v, np.array(t, dtype=np.uint32)


def torus(nu=24, nv=12, R=7.0, r=2.6, centre=(11.5, 11.5, 5.5)):
    """nu x nv quads split in two, about the z axis through `centre`."""
    u = np.arange(nu) * (2.0 * np.pi / nu)
    w = np.arange(nv) * (2.0 * np.pi / nv)
    uu, ww = np.meshgrid(u, w, indexing="ij")
    rad = R + r * np.cos(ww)
    v = np.stack([rad * np.cos(uu) + centre[0], rad * np.sin(uu) + centre[1], r * np.sin(ww) + centre[2]], axis=2).reshape(-1, 3)
    t = []
    for a in range(nu):
        for b in range(nv):
            p00, p10 = a * nv + b, ((a + 1) % nu) * nv + b
            p01, p11 = a * nv + (b + 1) % nv, ((a + 1) % nu) * nv + (b + 1) % nv
            t += [(p00, p10, p11), (p00, p11, p01)]
    return v.astype(np.float32), np.array(t, dtype=np.uint32)


def soup_of(vertices, triangles):
    """The triangles' corners, one after the other: (3 T, 3) float32."""
    return np.ascontiguousarray(np.asarray(vertices, dtype=np.float32)[np.asarray(triangles).astype(np.int64)].reshape(-1, 3))
