"""Mesh slicing in numpy and in plain Python: the contract of rm_slice_mesh restated twice, independently.

  slice_mesh(...)          vectorised numpy: edges by sorting, plane ranges by searchsorted, links as arrays, chains followed in a loop
  slice_mesh_by_walk(...)  plain Python: per plane from triangle to triangle through a dict of edges, points as Fractions that are
                           rounded where the contract rounds

Both return a dict: points (P, 3) float32, contours (C, 4) uint32 (first point, count, layer, closed), layer_first (n_layers + 1,)
uint32, counts (a dict of _ffi.MSLICE_COUNT_NAMES).  Also the planes, the loops as cyclic sequences, and the meshes the tests share."""
from fractions import Fraction

import numpy as np

import voxel_ref

COUNT_NAMES = ("triangles", "rejected", "paired_edges", "border_edges", "branch_edges", "segments", "points", "contours", "open_contours")
NIL = -1


def planes(heights, origin, step, axis):
    """P2 int64 (n_layers,): 2 floor(r) + 1 with r = (double(h) - double(o_w)) / double(s_w) * 64."""
    h = np.asarray(heights, dtype=np.float32).astype(np.float64)
    o = np.float64(np.float32(origin[axis]))
    s = np.float64(np.float32(step[axis]))
    return 2 * np.floor((h - o) / s * 64.0).astype(np.int64) + 1


def _accepted(vertices, triangles, origin, step):
    """(q int64 (V, 3), tri int64 (T, 3), ok bool (T,)): a triangle is rejected for an index out of range, two equal indices or a
    corner that does not snap."""
    q, valid = voxel_ref.snap(vertices, origin, step)
    tri = np.asarray(triangles).astype(np.int64).reshape(-1, 3)
    in_range = (tri < len(q)).all(axis=1)
    safe = np.where(tri < len(q), tri, 0)
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 2] != tri[:, 0])
    ok = in_range & distinct & valid[safe].all(axis=(1, 2))
    return q, tri, ok


def _world(g, o, s):
    """(float)((double)o + g / 64 * (double)s): g float64 array."""
    return (np.float64(np.float32(o)) + g / 64.0 * np.float64(np.float32(s))).astype(np.float32)


def slice_mesh(vertices, triangles, origin, step, axis, heights):
    w, u, v = axis, (axis + 1) % 3, (axis + 2) % 3
    q, tri, ok = _accepted(vertices, triangles, origin, step)
    P2 = planes(heights, origin, step, axis)
    assert np.all(np.diff(P2) > 0)
    n_layers, T = len(P2), len(tri)
    counts = dict.fromkeys(COUNT_NAMES, 0)
    counts["triangles"], counts["rejected"] = T, int((~ok).sum())
    # half-edges of the accepted triangles
    h_all = np.arange(3 * T, dtype=np.int64)
    h = h_all[np.repeat(ok, 3)]
    a, b = tri.reshape(-1)[h], tri[h // 3, (h % 3 + 1) % 3]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    order = np.lexsort((h, hi, lo))                                   # by edge, then by h
    hs, los, his, asc = h[order], lo[order], hi[order], (a < b)[order]
    first = np.ones(len(hs), dtype=bool)
    first[1:] = (los[1:] != los[:-1]) | (his[1:] != his[:-1])
    group = np.cumsum(first) - 1
    size = np.bincount(group) if len(hs) else np.zeros(0, dtype=np.int64)
    start = np.flatnonzero(first)
    two = size == 2
    paired = two.copy()
    paired[two] = asc[start[two]] != asc[start[two] + 1]
    counts["paired_edges"], counts["border_edges"] = int(paired.sum()), int((size == 1).sum())
    counts["branch_edges"] = int(len(size) - paired.sum() - (size == 1).sum())
    mate = np.full(3 * T, NIL, dtype=np.int64)
    p0 = start[paired]
    mate[hs[p0]], mate[hs[p0 + 1]] = hs[p0 + 1], hs[p0]
    canon = np.where((mate == NIL) | (h_all < mate), h_all, mate)     # (of the accepted half-edges)
    # plane ranges of every accepted half-edge, vertices on the canonical ones
    za, zb = q[a, w], q[b, w]
    k0 = np.searchsorted(P2, 2 * np.minimum(za, zb), side="right")
    k1 = np.searchsorted(P2, 2 * np.maximum(za, zb), side="left")
    cnt = np.maximum(k1 - k0, 0)
    is_canon = canon[h] == h
    cnt_c = np.where(is_canon, cnt, 0)
    estart = np.zeros(3 * T + 1, dtype=np.int64)
    full = np.zeros(3 * T, dtype=np.int64)
    full[h] = cnt_c
    estart[1:] = np.cumsum(full)
    k0_full = np.zeros(3 * T, dtype=np.int64)
    k0_full[h] = k0
    N = int(estart[-1])
    item_c = np.repeat(h[is_canon], cnt_c[is_canon])
    item_k = np.arange(N, dtype=np.int64) - estart[item_c] + k0_full[item_c]
    by_layer = np.lexsort((item_c, item_k))                           # ids: by (k, c)
    inv = np.empty(N, dtype=np.int64)
    inv[by_layer] = np.arange(N)
    vid_c, vid_k = item_c[by_layer], item_k[by_layer]

    def vertex_of(x, k):                                              # the id of the vertex of half-edge x's edge in plane k
        c = canon[x]
        return inv[estart[c] + k - k0_full[c]]
    # segments: every (accepted half-edge, plane it crosses), down ones and up ones aligned by (triangle, plane)
    xs = np.repeat(h, cnt)
    ks = np.arange(len(xs), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(k0, cnt)
    down = np.repeat(za > zb, cnt)
    nxt, prv = np.full(N, NIL, dtype=np.int64), np.full(N, NIL, dtype=np.int64)
    d, p = np.flatnonzero(down), np.flatnonzero(~down)
    d = d[np.lexsort((ks[d], xs[d] // 3))]
    p = p[np.lexsort((ks[p], xs[p] // 3))]
    assert len(d) == len(p) and np.array_equal(xs[d] // 3, xs[p] // 3) and np.array_equal(ks[d], ks[p])
    tail, head = vertex_of(xs[d], ks[d]), vertex_of(xs[p], ks[p])
    assert len(np.unique(tail)) == len(tail) and len(np.unique(head)) == len(head)
    nxt[tail], prv[head] = head, tail
    counts["segments"] = len(tail)
    # chains: open ones from the vertex no segment ends at, closed ones from their lowest id; ordered by first id
    seen = np.zeros(N, dtype=bool)
    chains = []
    for s0 in np.flatnonzero(prv == NIL):
        c, x = [], int(s0)
        while x != NIL:
            c.append(x)
            seen[x] = True
            x = int(nxt[x])
        chains.append((c, 0))
    for s0 in range(N):
        if not seen[s0]:
            c, x = [], s0
            while not seen[x]:
                c.append(x)
                seen[x] = True
                x = int(nxt[x])
            assert x == s0
            chains.append((c, 1))
    chains.sort(key=lambda e: e[0][0])
    seq = np.array([x for c, _ in chains for x in c], dtype=np.int64)
    contours = np.zeros((len(chains), 4), dtype=np.uint32)
    at = 0
    for i, (c, closed) in enumerate(chains):
        contours[i] = (at, len(c), vid_k[c[0]], closed)
        at += len(c)
    layer_first = np.searchsorted(contours[:, 2], np.arange(n_layers + 1), side="left").astype(np.uint32)
    # points
    c, k = vid_c[seq], vid_k[seq]
    ia, ib = tri.reshape(-1)[c], tri[c // 3, (c % 3 + 1) % 3]
    swap = q[ia, w] > q[ib, w]
    ia, ib = np.where(swap, ib, ia), np.where(swap, ia, ib)
    A, B, p2 = q[ia], q[ib], P2[k] if N else np.zeros(0, dtype=np.int64)
    num, den = p2 - 2 * A[:, w], 2 * (B[:, w] - A[:, w])
    pts = np.zeros((N, 3), dtype=np.float32)
    for ax in (u, v):
        g = A[:, ax].astype(np.float64) + ((B[:, ax] - A[:, ax]) * num).astype(np.float64) / den.astype(np.float64)
        pts[:, ax] = _world(g, origin[ax], step[ax])
    pts[:, w] = _world(p2.astype(np.float64) / 2.0, origin[w], step[w])
    counts["points"], counts["contours"] = N, len(chains)
    counts["open_contours"] = int(sum(1 for _, closed in chains if not closed))
    return {"points": pts, "contours": contours, "layer_first": layer_first, "counts": counts}


def _round_world(g, o, s):
    """g: an exact Fraction of a binary64 value -> the float32 world coordinate, every operation rounded once."""
    prod = float(g / 64 * Fraction(float(np.float32(s))))
    return np.float32(float(Fraction(float(np.float32(o))) + Fraction(prod)))


def slice_mesh_by_walk(vertices, triangles, origin, step, axis, heights):
    w, u, v = axis, (axis + 1) % 3, (axis + 2) % 3
    qn, trin, okn = _accepted(vertices, triangles, origin, step)
    q = [tuple(int(x) for x in row) for row in qn]
    tri = [tuple(int(x) for x in row) for row in trin]
    P2 = [int(x) for x in planes(heights, origin, step, axis)]
    counts = dict.fromkeys(COUNT_NAMES, 0)
    counts["triangles"], counts["rejected"] = len(tri), sum(1 for o in okn if not o)
    edges = {}                                                       # unordered pair -> its half-edges, ascending
    for t, (corners, ok) in enumerate(zip(tri, okn)):
        if ok:
            for s in range(3):
                a, b = corners[s], corners[(s + 1) % 3]
                edges.setdefault((min(a, b), max(a, b)), []).append(3 * t + s)

    def ascending(h):
        return tri[h // 3][h % 3] < tri[h // 3][(h % 3 + 1) % 3]
    canon = {}
    for hs in edges.values():
        if len(hs) == 2 and ascending(hs[0]) != ascending(hs[1]):
            counts["paired_edges"] += 1
            canon[hs[0]] = canon[hs[1]] = hs[0]
        else:
            counts["border_edges" if len(hs) == 1 else "branch_edges"] += 1
            for h in hs:
                canon[h] = h
    nxt, prv, verts = {}, {}, set()
    for k, p2 in enumerate(P2):
        for t, (corners, ok) in enumerate(zip(tri, okn)):
            if not ok:
                continue
            up = [2 * q[c][w] > p2 for c in corners]
            if all(up) or not any(up):
                continue
            tail = head = None
            for s in range(3):
                if up[s] and not up[(s + 1) % 3]:
                    tail = (k, canon[3 * t + s])
                if not up[s] and up[(s + 1) % 3]:
                    head = (k, canon[3 * t + s])
            assert tail not in nxt and head not in prv
            nxt[tail], prv[head] = head, tail
            verts.update((tail, head))
            counts["segments"] += 1
    chains, seen = [], set()
    for x in sorted(verts):
        if x not in prv:
            c = []
            while x is not None:
                c.append(x)
                seen.add(x)
                x = nxt.get(x)
            chains.append((c, 0))
    for x in sorted(verts):
        if x not in seen:
            c = []
            while x not in seen:
                c.append(x)
                seen.add(x)
                x = nxt[x]
            chains.append((c, 1))
    chains.sort(key=lambda e: e[0][0])
    pts, contours = [], []
    for c, closed in chains:
        contours.append((len(pts), len(c), c[0][0], closed))
        for k, h in c:
            ia, ib = tri[h // 3][h % 3], tri[h // 3][(h % 3 + 1) % 3]
            if q[ia][w] > q[ib][w]:
                ia, ib = ib, ia
            A, B, p2 = q[ia], q[ib], P2[k]
            out = [None] * 3
            for ax in (u, v):
                quot = float(Fraction((B[ax] - A[ax]) * (p2 - 2 * A[w]), 2 * (B[w] - A[w])))
                g = float(Fraction(A[ax]) + Fraction(quot))
                out[ax] = _round_world(Fraction(g), origin[ax], step[ax])
            out[w] = _round_world(Fraction(p2, 2), origin[w], step[w])
            pts.append(out)
    counts["points"], counts["contours"] = len(pts), len(chains)
    counts["open_contours"] = sum(1 for _, closed in chains if not closed)
    layers = [cn[2] for cn in contours]
    layer_first = np.searchsorted(np.array(layers, dtype=np.int64), np.arange(len(P2) + 1), side="left").astype(np.uint32)
    return {"points": np.array(pts, dtype=np.float32).reshape(-1, 3), "contours": np.array(contours, dtype=np.uint32).reshape(-1, 4),
            "layer_first": layer_first, "counts": counts}


# ---- what the tests compare ---------------------------------------------------------------------------------------------------------
def area(result, contour, axis):
    """The float64 shoelace area of a contour in (u, v), seen from +w."""
    first, count = int(result["contours"][contour][0]), int(result["contours"][contour][1])
    p = result["points"][first:first + count][:, [(axis + 1) % 3, (axis + 2) % 3]].astype(np.float64)
    x, y = p[:, 0], p[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def canonical_loops(result):
    """Per layer the sorted list of its contours as (closed, point bytes), a closed one rotated to start at its least point: equal
    for two results whose loops are the same cyclic sequences in whatever order and from whatever start."""
    out = []
    lf = result["layer_first"]
    for k in range(len(lf) - 1):
        loops = []
        for c in range(int(lf[k]), int(lf[k + 1])):
            first, count, _, closed = (int(x) for x in result["contours"][c])
            rows = [r.tobytes() for r in result["points"][first:first + count]]
            if closed:
                i = rows.index(min(rows))
                rows = rows[i:] + rows[:i]
            loops.append((closed, tuple(rows)))
        out.append(sorted(loops))
    return out


def box_fin():
    """voxel_ref.box with the fin (0, 1, 6): the edge (0, 1) gets a third face, (1, 6) a third face as well, (6, 0) is new."""
    v, t = voxel_ref.box((2, 3, 4), (10, 9, 8))
    return v, np.concatenate([t, np.array([(0, 1, 6)], dtype=np.uint32)])


def cases():
    """name -> (vertices, triangles, heights): the meshes of the CPU and GPU tests, origin 0 and step 1."""
    bv, bt = voxel_ref.box((2, 3, 4), (10, 9, 8))
    fv, ft = box_fin()
    tv, tt = voxel_ref.torus()
    sv, stt = voxel_ref.icosphere(3, 9.3, (12.1, 11.7, 12.4))
    return {"box": (bv, bt, [3, 5, 7, 20]), "open_box": (bv, np.delete(bt, [2, 3], axis=0), [5]), "torus": (tv, tt, [5.5]),
            "sphere": (sv, stt, np.arange(2, 22, 0.5)), "fin": (fv, ft, [5])}
