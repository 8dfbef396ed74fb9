"""A numpy restatement of the slicing contract, for the tests: the square case table, the lattice of
a layer, and the extraction of ordered contours from lattice distances.  Written from the contract, not from
csrc/rm_slice.h: the table walks each cell's boundary instead of testing sides with cross products, and chains are
followed with a plain loop instead of ranked.  Test infrastructure only; binary32 arithmetic throughout, one rounded
operation at a time (numpy never fuses)."""
import numpy as np

F = np.float32
NO_EDGE = 0xFFFFFFFF
NIL = -1

# the corners of a cell counter-clockwise seen from +w (u to the right, v up), corner c at (c & 1, c >> 1)
CYCLE = (0, 1, 3, 2)
# the cell edge between two neighbouring corners: 0 bottom, 1 top, 2 left, 3 right
EDGE_OF = {frozenset((0, 1)): 0, frozenset((2, 3)): 1, frozenset((0, 2)): 2, frozenset((1, 3)): 3}


def case_segments(case):
    """The directed segments (tail edge, head edge) of one case, ordered by tail edge."""
    inside = [(case >> c) & 1 for c in range(4)]
    start = next((q for q in range(4) if not inside[CYCLE[q]]), None)
    if start is None:
        return []
    segs, enter = [], None
    for q in range(start, start + 4):
        a, b = CYCLE[q % 4], CYCLE[(q + 1) % 4]
        e = EDGE_OF[frozenset((a, b))]
        if not inside[a] and inside[b]:
            enter = e                       # a run of inside corners is entered through this edge ...
        elif inside[a] and not inside[b]:
            assert enter is not None
            segs.append((e, enter))         # ... and left through this one: the segment runs from here back to the entry
            enter = None
    return sorted(segs)


def case_table():
    """16 x 5 uint32, the layout of rm_slice_case_table."""
    t = np.full((16, 5), NO_EDGE, dtype=np.uint32)
    for case in range(16):
        segs = case_segments(case)
        t[case, 0] = len(segs)
        for k, (tail, head) in enumerate(segs):
            t[case, 1 + 2 * k], t[case, 2 + 2 * k] = tail, head
    return t


_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = case_table()
    return _TABLE


# ---- lattice -------------------------------------------------------------------------------------------------------------
def in_plane_axes(axis):
    return (axis + 1) % 3, (axis + 2) % 3


def axis_coords(origin, step, n):
    """o + (float)i * s: one rounded product, one rounded sum."""
    return F(origin) + np.arange(n, dtype=np.float64).astype(F) * F(step)


def layer_points(axis, origin_uv, step_uv, shape_uv, height):
    """(nu*nv, 3) float32 world positions of a layer's lattice points, in the order i + nu * j."""
    u, v = in_plane_axes(axis)
    nu, nv = shape_uv
    cu, cv = axis_coords(origin_uv[0], step_uv[0], nu), axis_coords(origin_uv[1], step_uv[1], nv)
    p = np.empty((nv, nu, 3), dtype=F)
    p[:, :, u] = cu[None, :]
    p[:, :, v] = cv[:, None]
    p[:, :, axis] = F(height)
    return p.reshape(-1, 3)


# ---- one layer -------------------------------------------------------------------------------------------------------------
def layer_cases(dist, level=0.0):
    """The case of every cell of a layer: (nv - 1, nu - 1)."""
    with np.errstate(invalid="ignore"):
        inside = np.ascontiguousarray(dist, dtype=F) < F(level)
    nv, nu = inside.shape
    case = np.zeros((nv - 1, nu - 1), dtype=np.int64)
    for c in range(4):
        case |= inside[(c >> 1):(c >> 1) + nv - 1, (c & 1):(c & 1) + nu - 1].astype(np.int64) << c
    return case


def layer_links(dist, origin_uv, step_uv, level=0.0):
    """dist: (nv, nu) float32.  Returns (uv (V, 2) float32 in vertex id order, next (V,), prev (V,)) with NIL = -1."""
    d = np.ascontiguousarray(dist, dtype=F)
    nv, nu = d.shape
    lev = F(level)
    cu, cv = axis_coords(origin_uv[0], step_uv[0], nu), axis_coords(origin_uv[1], step_uv[1], nv)
    with np.errstate(invalid="ignore"):
        inside = d < lev                                            # NaN: outside
    cross = np.zeros((nv, nu, 2), dtype=bool)                       # [j, i, a]: the edge from (i, j) along in-plane axis a
    cross[:, :-1, 0] = inside[:, :-1] != inside[:, 1:]
    cross[:-1, :, 1] = inside[:-1, :] != inside[1:, :]
    flat = cross.reshape(-1, 2)
    counts = flat.sum(axis=1).astype(np.int64)
    vbase = np.cumsum(counts) - counts
    q, a = np.nonzero(flat)                                         # vertices in (point, axis) order
    i, j = q % nu, q // nu
    da = d.ravel()[q]
    db = d[j + (a == 1), i + (a == 0)]
    with np.errstate(all="ignore"):
        t = (da - lev) / (da - db)
        ua, ub = cu[i], cu[np.minimum(i + 1, nu - 1)]
        va, vb = cv[j], cv[np.minimum(j + 1, nv - 1)]
        uv = np.stack([np.where(a == 0, ua + t * (ub - ua), ua), np.where(a == 1, va + t * (vb - va), va)], axis=1).astype(F)
    V = len(q)
    nxt = np.full(V, NIL, dtype=np.int64)
    prv = np.full(V, NIL, dtype=np.int64)
    case = layer_cases(d, level).ravel()
    tab = table().astype(np.int64)
    cells = np.arange(len(case))
    ci, cj = cells % (nu - 1), cells // (nu - 1)

    def vertex_of(edge, sel):
        # the lattice point the edge starts at: top is the u-edge of (i, j + 1), right the v-edge of (i + 1, j)
        pt = (ci[sel] + (edge == 3)) + nu * (cj[sel] + (edge == 1))
        return vbase[pt] + ((edge >> 1) == 1) * flat[pt, 0]
    for k in range(2):
        sel = tab[case, 0] > k
        tail = vertex_of(tab[case[sel], 1 + 2 * k], sel)
        head = vertex_of(tab[case[sel], 2 + 2 * k], sel)
        assert np.all(nxt[tail] == NIL) and np.all(prv[head] == NIL)
        assert len(np.unique(tail)) == len(tail) and len(np.unique(head)) == len(head)
        nxt[tail] = head
        prv[head] = tail
    return uv, nxt, prv


def layer_chains(nxt, prv):
    """The contours of one layer as (vertex ids in order, closed), in canonical order: by the id of the first vertex."""
    V = len(nxt)
    nxt_l = nxt.tolist()
    seen = np.zeros(V, dtype=bool)
    out = []
    for first in np.nonzero(prv == NIL)[0].tolist():                # open: from the vertex no segment ends at
        ids, v = [], first
        while v != NIL:
            assert not seen[v]
            seen[v] = True
            ids.append(v)
            v = nxt_l[v]
        out.append((first, ids, False))
    for first in range(V):                                          # closed: in id order the first unseen vertex is the lowest
        if seen[first]:
            continue
        ids, v = [], first
        while not seen[v]:
            seen[v] = True
            ids.append(v)
            v = nxt_l[v]
        assert v == first, "segments do not close into a loop"
        out.append((first, ids, True))
    out.sort(key=lambda c: c[0])
    return [(ids, closed) for _, ids, closed in out]


# ---- a stack of layers -------------------------------------------------------------------------------------------------------
def slice_contours(dists, axis, origin_uv, step_uv, heights, level=0.0):
    """dists: per layer a (nv, nu) float32 array of lattice distances.  Returns (points (P, 3) float32, contours (C, 4)
    uint32, layer_first (n_layers + 1,) uint32) as rm_read_slices does."""
    u, v = in_plane_axes(axis)
    pts, cons, layer_first = [], [], [0]
    P = 0
    for k, d in enumerate(dists):
        uv, nxt, prv = layer_links(d, origin_uv, step_uv, level)
        for ids, closed in layer_chains(nxt, prv):
            w = np.empty((len(ids), 3), dtype=F)
            w[:, u], w[:, v], w[:, axis] = uv[ids, 0], uv[ids, 1], F(heights[k])
            pts.append(w)
            cons.append((P, len(ids), k, int(closed)))
            P += len(ids)
        layer_first.append(len(cons))
    points = np.concatenate(pts) if pts else np.zeros((0, 3), dtype=F)
    return points, np.asarray(cons, dtype=np.uint32).reshape(-1, 4), np.asarray(layer_first, dtype=np.uint32)


def shoelace(uv):
    """Signed area of a closed polygon, float64: positive for counter-clockwise."""
    p = np.asarray(uv, dtype=np.float64)
    x, y = p[:, 0], p[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
