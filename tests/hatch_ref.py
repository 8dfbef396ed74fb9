"""Hatching in numpy and in plain Python: the contract of rm_hatch_slices restated twice, independently.

  hatch(...)          vectorised numpy: line ranges by searchsorted on c, one stable argsort of the 64-bit key
  hatch_by_walk(...)  plain Python: per segment, per line, the half-open rule literally; Python floats (binary64) and numpy.float32
                      roundings; sorted by (key, enumeration index)

Both take the arrays rm_read_slices gives (points (P, 3) float32, contours (C, 4) uint32), the number of layers, the slicing axis,
lines (n_layers, 4) float32 = (dx, dy, offset, spacing) per layer and n_lines, and return a dict: segments (H, 4) float32
(u, v of one end, u, v of the other), line (H,) uint32, layer_first (n_layers + 1,) uint32, counts (a dict of COUNT_NAMES).
Also: the tolerance of a crossing's normal coordinate, an exact even-odd inside test, and slices of the meshes the tests share."""
from fractions import Fraction

import numpy as np

import mesh_slice_ref

COUNT_NAMES = ("segments_in", "crossings", "segments", "lines_hit", "odd_lines")
O, S = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def sliced(name, axis):
    """mesh_slice_ref.slice_mesh of a mesh_slice_ref.cases() mesh, origin 0 and step 1: (result, n_layers)."""
    v, t, h = mesh_slice_ref.cases()[name]
    return mesh_slice_ref.slice_mesh(v, t, O, S, axis, h), len(h)


def as_lines(line, n_layers):
    """One (dx, dy, offset, spacing) for every layer."""
    return np.tile(np.asarray(line, dtype=np.float32).reshape(1, 4), (n_layers, 1))


def line_values(lines, k, n_lines):
    """c_j float64 (n_lines,): (double)offset + (double)j * (double)spacing."""
    off, sp = np.float64(lines[k, 2]), np.float64(lines[k, 3])
    return off + np.arange(n_lines, dtype=np.float64) * sp


def normal_coordinate(pu, pv, dx, dy):
    """s float64: (double)P_v (double)dx - (double)P_u (double)dy; pu, pv float32 arrays."""
    return pv.astype(np.float64) * np.float64(dx) - pu.astype(np.float64) * np.float64(dy)


def key32(r):
    """The order-preserving map of float32 r onto uint32."""
    b = np.asarray(r, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def tails_and_heads(contours, n_points):
    """(tail, head, layer) int64: the segments in the order of their ids (= tail points)."""
    tail, head, layer = [], [], []
    for f, n, k, closed in np.asarray(contours).astype(np.int64).reshape(-1, 4):
        i = np.arange(f, f + (n if closed else n - 1), dtype=np.int64)
        tail.append(i)
        head.append(f + (i - f + 1) % n)
        layer.append(np.full(len(i), k, dtype=np.int64))
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, dtype=np.int64)  # noqa: E731
    return cat(tail), cat(head), cat(layer)


def _pair(key, X, n_layers, n_lines, zigzag, counts):
    """Sorted crossings (key uint64, X (N, 2) float32) -> segments, line, layer_first; fills the counts."""
    L = (key >> np.uint64(32)).astype(np.int64)
    N = len(L)
    start = np.searchsorted(L, L, side="left")
    end = np.searchsorted(L, L, side="right")
    rank = np.arange(N, dtype=np.int64) - start
    head = (rank % 2 == 0) & (np.arange(N) + 1 < end)
    counts["lines_hit"] = int(np.count_nonzero(rank == 0))
    counts["odd_lines"] = int(np.count_nonzero((rank == 0) & ((end - start) % 2 == 1)))
    q = np.flatnonzero(head)
    pos = np.arange(len(q), dtype=np.int64)
    a, b = X[q], X[q + 1] if len(q) else X[q]
    if zigzag:
        first = np.searchsorted(L[q], L[q], side="left")             # the first segment of the line, and how many it has
        m = np.searchsorted(L[q], L[q], side="right") - first
        odd = (L[q] % n_lines) % 2 == 1
        pos = np.where(odd, first + m - 1 - (pos - first), pos)
        a, b = np.where(odd[:, None], b, a), np.where(odd[:, None], a, b)
    seg = np.zeros((len(q), 4), dtype=np.float32)
    line = np.zeros(len(q), dtype=np.uint32)
    seg[pos, :2], seg[pos, 2:], line[pos] = a, b, L[q].astype(np.uint32)
    counts["segments"] = len(q)
    layer_first = np.searchsorted(L[q], np.arange(n_layers + 1, dtype=np.int64) * n_lines, side="left").astype(np.uint32)
    return seg, line, layer_first


def hatch(points, contours, n_layers, axis, lines, n_lines, zigzag=False):
    u, v = (axis + 1) % 3, (axis + 2) % 3
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    lines = np.asarray(lines, dtype=np.float32).reshape(n_layers, 4)
    tail, head, layer = tails_and_heads(contours, len(pts))
    counts = dict.fromkeys(COUNT_NAMES, 0)
    counts["segments_in"] = len(tail)
    dx, dy = lines[layer, 0], lines[layer, 1]
    sT, sH = normal_coordinate(pts[tail, u], pts[tail, v], dx, dy), normal_coordinate(pts[head, u], pts[head, v], dx, dy)
    ok = np.isfinite(sT) & np.isfinite(sH) & (sT != sH)
    ia, ib = np.where(sT < sH, tail, head), np.where(sT < sH, head, tail)
    sA, sB = np.minimum(sT, sH), np.maximum(sT, sH)
    j0, j1 = np.zeros(len(tail), dtype=np.int64), np.zeros(len(tail), dtype=np.int64)
    for k in range(n_layers):
        m = ok & (layer == k)
        c = line_values(lines, k, n_lines)
        j0[m], j1[m] = np.searchsorted(c, sA[m], side="left"), np.searchsorted(c, sB[m], side="left")
    cnt = j1 - j0
    N = int(cnt.sum())
    counts["crossings"] = N
    seg = np.repeat(np.arange(len(tail), dtype=np.int64), cnt)
    j = np.arange(N, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(j0, cnt)
    k = layer[seg]
    cj = lines[k, 2].astype(np.float64) + j.astype(np.float64) * lines[k, 3].astype(np.float64)
    with np.errstate(all="ignore"):
        t = (cj - sA[seg]) / (sB[seg] - sA[seg])
    X = np.zeros((N, 2), dtype=np.float32)
    for col, ax in enumerate((u, v)):
        A, B = pts[ia[seg], ax].astype(np.float64), pts[ib[seg], ax].astype(np.float64)
        X[:, col] = (A + t * (B - A)).astype(np.float32)
    r = (X[:, 0].astype(np.float64) * lines[k, 0].astype(np.float64) + X[:, 1].astype(np.float64) * lines[k, 1].astype(np.float64)).astype(np.float32)
    key = ((k * n_lines + j).astype(np.uint64) << np.uint64(32)) | key32(r).astype(np.uint64)
    order = np.argsort(key, kind="stable")
    segs, line, layer_first = _pair(key[order], X[order], n_layers, n_lines, zigzag, counts)
    return {"segments": segs, "line": line, "layer_first": layer_first, "counts": counts, "ties": int(N - len(np.unique(key)))}


def hatch_by_walk(points, contours, n_layers, axis, lines, n_lines, zigzag=False):
    u, v = (axis + 1) % 3, (axis + 2) % 3
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    lines = np.asarray(lines, dtype=np.float32).reshape(n_layers, 4)
    counts = dict.fromkeys(COUNT_NAMES, 0)
    crossings = []                                                   # (key, enumeration index, X_u, X_v)
    for f, n, k, closed in [tuple(int(x) for x in row) for row in np.asarray(contours).reshape(-1, 4)]:
        dx, dy, off, sp = (float(x) for x in lines[k])
        for i in range(f, f + n):
            if not closed and i == f + n - 1:
                continue
            counts["segments_in"] += 1
            h = f + (i - f + 1) % n
            ends = []
            for p in (i, h):
                pu, pv = float(pts[p, u]), float(pts[p, v])
                ends.append((pv * dx - pu * dy, pu, pv))
            (sA, au, av), (sB, bu, bv) = sorted(ends, key=lambda e: e[0])
            if not (np.isfinite(sA) and np.isfinite(sB)) or sA == sB:
                continue
            for j in range(n_lines):
                cj = off + float(j) * sp
                if not sA <= cj < sB:
                    continue
                t = (cj - sA) / (sB - sA)
                xu, xv = np.float32(au + t * (bu - au)), np.float32(av + t * (bv - av))
                r = np.float32(float(xu) * dx + float(xv) * dy)
                bits = int(r.view(np.uint32))
                k32 = bits ^ (0xFFFFFFFF if bits >> 31 else 0x80000000)
                crossings.append((((k * n_lines + j) << 32) | k32, len(crossings), xu, xv))
    counts["crossings"] = len(crossings)
    crossings.sort(key=lambda e: (e[0], e[1]))
    by_line = {}
    for key, _, xu, xv in crossings:
        by_line.setdefault(key >> 32, []).append((xu, xv))
    segs, line = [], []
    for L in sorted(by_line):
        xs = by_line[L]
        counts["lines_hit"] += 1
        counts["odd_lines"] += len(xs) % 2
        mine = [(xs[2 * i] + xs[2 * i + 1]) for i in range(len(xs) // 2)]
        if zigzag and (L % n_lines) % 2 == 1:
            mine = [(s[2], s[3], s[0], s[1]) for s in reversed(mine)]
        segs += mine
        line += [L] * len(mine)
    counts["segments"] = len(segs)
    layer_first = np.searchsorted(np.array(line, dtype=np.int64), np.arange(n_layers + 1, dtype=np.int64) * n_lines, side="left")
    return {"segments": np.array(segs, dtype=np.float32).reshape(-1, 4), "line": np.array(line, dtype=np.uint32),
            "layer_first": layer_first.astype(np.uint32), "counts": counts}


# ---- what the tests compare ---------------------------------------------------------------------------------------------------------
def same(a, b):
    """Whether two results are equal to the last bit."""
    return (a["counts"] == b["counts"] and a["segments"].shape == b["segments"].shape
            and np.array_equal(a["segments"].view(np.uint32), b["segments"].view(np.uint32))
            and np.array_equal(a["line"], b["line"]) and np.array_equal(a["layer_first"], b["layer_first"]))


def lengths(result, dx, dy):
    """The float64 lengths of the hatch segments."""
    s = result["segments"].astype(np.float64)
    return np.hypot(s[:, 2] - s[:, 0], s[:, 3] - s[:, 1])


def s_tolerance(m_uv, dx, dy):
    """How far s of an end of a hatch segment may lie from its line's c, for in-plane coordinates of magnitude <= m_uv.

    With A, B the ends of the contour segment and D = |dx| + |dy|, e = 2^-53, q = 2^-24:
      item 2   s(P) carries one rounding: |s - exact| <= e |s| <= e m D for every point, so the exact s of A and B differ from the
               values the crossing was found with by at most e m D each;
      item 6   t in [0, 1) has a relative error of at most 3 e (two differences and a quotient), B_a - A_a one of e, the product
               and the sum one more each: the binary64 coordinate is within 8 e m of the exact point of the line, and the
               conversion to binary32 moves it by at most q m: in s that is (8 e + q) m D;
      the s of the binary32 point itself is rounded once more: e m D.
    The sum is below (q + 12 e) m D; 2 q m D -- "one binary32 ulp-scaled" -- is what the tests assert."""
    return 2.0 * 2.0 ** -24 * m_uv * (abs(float(dx)) + abs(float(dy)))


def inside_even_odd(points, contours, layer, axis, x, y):
    """The even-odd rule for the point (x, y) (Fractions) against the closed contours of `layer`, exactly: a ray towards +u."""
    u, v = (axis + 1) % 3, (axis + 2) % 3
    inside = False
    for f, n, k, closed in [tuple(int(q) for q in row) for row in np.asarray(contours).reshape(-1, 4)]:
        if k != layer or not closed:
            continue
        for i in range(n):
            a, b = points[f + i], points[f + (i + 1) % n]
            ax, ay, bx, by = (Fraction(float(a[u])), Fraction(float(a[v])), Fraction(float(b[u])), Fraction(float(b[v])))
            if (ay > y) != (by > y) and x < ax + (y - ay) * (bx - ax) / (by - ay):
                inside = not inside
    return inside


def distance_to_outline(points, contours, layer, axis, x, y):
    """The float64 distance of (x, y) from the nearest contour segment of `layer`."""
    u, v = (axis + 1) % 3, (axis + 2) % 3
    tail, head, lay = tails_and_heads(contours, len(points))
    m = lay == layer
    a, b = points[tail[m]][:, [u, v]].astype(np.float64), points[head[m]][:, [u, v]].astype(np.float64)
    d = b - a
    p = np.array([x, y], dtype=np.float64)
    with np.errstate(all="ignore"):
        t = np.clip(np.nan_to_num(((p - a) * d).sum(axis=1) / (d * d).sum(axis=1)), 0.0, 1.0)
    return float(np.min(np.hypot(*(a + t[:, None] * d - p).T))) if len(a) else float("inf")
