"""A numpy restatement of the mesh-export contract, for the tests: the cube case table, lattice
coordinates, and the extraction of vertices and triangles from lattice distances.  Written from the contract, not from
csrc/rm_mesh.h: the table walks each face's boundary instead of testing sides with cross products.  Test infrastructure
only; binary32 arithmetic throughout, one rounded operation at a time (numpy never fuses)."""
import math

import numpy as np

F = np.float32
NO_EDGE = 0xFFFFFFFF


# ---- the case table -----------------------------------------------------------------------------------------------------
def corner_pos(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_ends(e):
    """(corner at 0 on the edge's axis, corner at 1)."""
    a = e >> 2
    others = [x for x in range(3) if x != a]          # increasing axis order: bit 0 for the lower one
    pos = [0, 0, 0]
    pos[others[0]] = e & 1
    pos[others[1]] = (e >> 1) & 1
    c0 = pos[0] | pos[1] << 1 | pos[2] << 2
    return c0, c0 | (1 << a)


EDGE_OF = {frozenset(edge_ends(e)): e for e in range(12)}


def face_cycles():
    """The corners of each of the six faces in counter-clockwise order seen from outside the cube."""
    out = []
    for f in range(3):
        for s in (0, 1):
            n = [0.0, 0.0, 0.0]
            n[f] = 1.0 if s else -1.0
            u = [0.0, 0.0, 0.0]
            u[(f + 1) % 3] = 1.0
            v = np.cross(n, u)                        # (u, v, n) right-handed: angles grow counter-clockwise seen from +n
            cs = [c for c in range(8) if corner_pos(c)[f] == s]
            ang = {c: math.atan2(np.dot(np.subtract(corner_pos(c), 0.5), v), np.dot(np.subtract(corner_pos(c), 0.5), u))
                   for c in cs}
            out.append(sorted(cs, key=ang.get))
    return out


def case_triangles(case):
    """The triangles (edge triples) of one case by the contract's rule."""
    inside = [(case >> c) & 1 for c in range(8)]
    nxt = {}
    for cyc in face_cycles():
        # walking the boundary counter-clockwise, a run of inside corners is entered through one edge and left through the
        # next: the segment between them has the run on its right
        enter = None
        start = next((q for q in range(4) if not inside[cyc[q]]), None)
        if start is None:
            continue
        for q in range(start, start + 4):
            a, b = cyc[q % 4], cyc[(q + 1) % 4]
            e = EDGE_OF[frozenset((a, b))]
            if not inside[a] and inside[b]:
                enter = e
            elif inside[a] and not inside[b]:
                assert enter is not None and enter not in nxt
                nxt[enter] = e
    tris, seen = [], set()
    for e0 in sorted(nxt):
        if e0 in seen:
            continue
        loop, e = [], e0
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == e0, "segments do not close into a loop"
        tris += [(loop[0], loop[k], loop[k + 1]) for k in range(1, len(loop) - 1)]
    return tris


def case_table():
    """256 x 16 uint32, the layout of rm_mesh_case_table."""
    t = np.full((256, 16), NO_EDGE, dtype=np.uint32)
    for case in range(256):
        tris = case_triangles(case)
        t[case, 0] = len(tris)
        for k, tri in enumerate(tris):
            t[case, 1 + 3 * k:4 + 3 * k] = tri
    return t


_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = case_table()
    return _TABLE


# ---- lattice and extraction --------------------------------------------------------------------------------------------
def axis_coords(origin, step, shape):
    """Per axis, the coordinates of its lattice points: o + (float)i * s (one rounded product, one rounded sum)."""
    return [F(origin[a]) + np.arange(shape[a], dtype=np.float64).astype(F) * F(step[a]) for a in range(3)]


def lattice_points(origin, step, shape):
    """(nx*ny*nz, 3) float32 in linear order (x fastest)."""
    xs, ys, zs = axis_coords(origin, step, shape)
    z, y, x = np.meshgrid(zs, ys, xs, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


def extract(dist, origin, step, level=0.0):
    """dist: (nz, ny, nx) float32 lattice values.  Returns (vertices (V, 3) float32, triangles (T, 3) uint32)."""
    d = np.ascontiguousarray(dist, dtype=F)
    nz, ny, nx = d.shape
    lev = F(level)
    coords = axis_coords(origin, step, (nx, ny, nz))
    with np.errstate(invalid="ignore"):
        inside = d < lev                                              # NaN: outside
    cross = np.zeros((nz, ny, nx, 3), dtype=bool)                      # [k, j, i, axis]: the edge from (i, j, k) along axis
    cross[:, :, :-1, 0] = inside[:, :, :-1] != inside[:, :, 1:]
    cross[:, :-1, :, 1] = inside[:, :-1, :] != inside[:, 1:, :]
    cross[:-1, :, :, 2] = inside[:-1, :, :] != inside[1:, :, :]
    flat = cross.reshape(-1, 3)
    counts = flat.sum(axis=1).astype(np.int64)
    vbase = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    # vertices in (point, axis) order
    p, a = np.nonzero(flat)
    i, j, k = p % nx, (p // nx) % ny, p // (nx * ny)
    ijk = np.stack([i, j, k], axis=1)
    step1 = np.eye(3, dtype=np.int64)[a]
    da = d.ravel()[p]
    q = ijk + step1
    db = d[q[:, 2], q[:, 1], q[:, 0]]
    with np.errstate(all="ignore"):
        t = (da - lev) / (da - db)
    verts = np.empty((len(p), 3), dtype=F)
    for ax in range(3):
        xa = coords[ax][ijk[:, ax]]
        on = a == ax
        xb = coords[ax][np.minimum(ijk[:, ax] + 1, len(coords[ax]) - 1)]
        with np.errstate(all="ignore"):
            moved = xa + t * (xb - xa)
        verts[:, ax] = np.where(on, moved, xa)
    # triangles: cells by linear cell index, then table order
    case = np.zeros((nz - 1, ny - 1, nx - 1), dtype=np.int64)
    for c in range(8):
        ox, oy, oz = corner_pos(c)
        case |= inside[oz:oz + nz - 1, oy:oy + ny - 1, ox:ox + nx - 1].astype(np.int64) << c
    case = case.ravel()
    tab = table()
    ntri = tab[case, 0].astype(np.int64)
    cells = np.repeat(np.arange(len(case)), ntri)
    first = np.repeat(np.cumsum(ntri) - ntri, ntri)
    tri_in_cell = np.arange(len(cells)) - first
    ci, cj, ck = cells % (nx - 1), (cells // (nx - 1)) % (ny - 1), cells // ((nx - 1) * (ny - 1))
    tris = np.empty((len(cells), 3), dtype=np.uint32)
    for m in range(3):
        e = tab[case[cells], 1 + 3 * tri_in_cell + m].astype(np.int64)
        ax = e >> 2
        c0 = np.array([edge_ends(x)[0] for x in range(12)], dtype=np.int64)[e]
        qi, qj, qk = ci + (c0 & 1), cj + ((c0 >> 1) & 1), ck + ((c0 >> 2) & 1)
        qp = qi + nx * (qj + ny * qk)
        below = np.zeros(len(e), dtype=np.int64)
        for lower in range(2):
            below += (flat[qp, lower] & (lower < ax)).astype(np.int64)
        tris[:, m] = (vbase[qp] + below).astype(np.uint32)
    return verts, tris


# ---- topology ------------------------------------------------------------------------------------------------------------
def directed_edges(tris):
    t = np.asarray(tris, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def directed_edges_balance(tris):
    """Every directed edge (u, v) occurs as often as (v, u): closed and consistently oriented."""
    de = directed_edges(tris)
    if len(de) == 0:
        return True
    fwd, nf = np.unique(de, axis=0, return_counts=True)
    rev, nr = np.unique(de[:, ::-1], axis=0, return_counts=True)
    return bool(np.array_equal(fwd, rev) and np.array_equal(nf, nr))


def is_closed_manifold(tris):
    """Each directed edge occurs once and its reverse once: a closed, oriented 2-manifold."""
    de = directed_edges(tris)
    _, n = np.unique(de, axis=0, return_counts=True)
    return bool(np.all(n == 1) and directed_edges_balance(tris))


def euler_characteristic(tris):
    t = np.asarray(tris, dtype=np.int64)
    de = directed_edges(t)
    und = np.unique(np.sort(de, axis=1), axis=0)
    return len(np.unique(t)) - len(und) + len(t)


def signed_volume(verts, tris):
    v = np.asarray(verts, dtype=np.float64)[np.asarray(tris, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)
