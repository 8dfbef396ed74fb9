"""A numpy restatement of the layer-regions-and-islands contract, for the tests, in two independent forms:
per_point(occ, ...) follows the definitions word for word -- per layer a flood fill with an explicit stack in the caller's frame,
per point a loop over the disc of the layer below --; layerwise(occ, ...) turns the lattice so that the height is the first axis
and works on whole layers: minimum propagation over shifted arrays for the regions, shifted label arrays for the links.  Both
return a Result: counts (COUNT_NAMES -> int), rows uint32 (REGIONS, 12), labels uint32 (nz, ny, nx), mask uint8 (nz, ny, nx),
profile uint32 (n_a, 4).  Written from the contract, not from the kernels.  Test infrastructure only."""
import collections

import numpy as np

import mass_ref
from support_ref import UPS, _shifted, disc, up_index  # noqa: F401

COUNT_NAMES = ("points", "plate", "regions", "base_regions", "islands", "island_points", "merges", "max_layer_regions")
ROW_NAMES = ("layer", "first", "points", "supported", "sum_a", "sum_b", "min_a", "max_a", "min_b", "max_b", "below_min", "below_max")
LAYER, FIRST, POINTS, SUPPORTED, SUM_A, SUM_B, MIN_A, MAX_A, MIN_B, MAX_B, BELOW_MIN, BELOW_MAX = range(12)
Result = collections.namedtuple("Result", "counts rows labels mask profile")


def _finish(rows, labels, inside, h0, height_of_axis):
    """counts, mask and profile from the rows and the label volume.  height_of_axis: (numpy axis of the heights, reversed)."""
    npaxis, neg = height_of_axis
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, 12)
    nh = inside.shape[npaxis]
    island = (rows[:, LAYER] > h0) & (rows[:, BELOW_MIN] == 0)
    merge = rows[:, BELOW_MIN] != rows[:, BELOW_MAX]
    mask = inside.astype(np.uint8)
    if len(rows):
        mask[np.concatenate([[False], island])[labels]] = 2
    profile = np.zeros((nh, 4), dtype=np.uint32)
    ins_h = np.moveaxis(inside, npaxis, 0)
    ins_h = ins_h[::-1] if neg else ins_h
    profile[:, 0] = ins_h.reshape(nh, -1).sum(axis=1)
    for r in range(len(rows)):
        h = int(rows[r, LAYER])
        profile[h, 1] += 1
        if island[r]:
            profile[h, 2] += 1
            profile[h, 3] += rows[r, POINTS]
    counts = {"points": int(profile[:, 0].sum()), "plate": int(h0), "regions": len(rows), "base_regions": int(profile[h0, 1]),
              "islands": int(island.sum()), "island_points": int(rows[island, POINTS].sum()), "merges": int(merge.sum()),
              "max_layer_regions": int(profile[:, 1].max())}
    return Result(counts, rows, labels, mask, profile)


# ---- form (a): per point ----------------------------------------------------------------------------------------------------------
def per_point(occ, up="+z", r2=1, plate=None):
    inside = np.asarray(occ) != 0
    nz, ny, nx = inside.shape
    n = (nx, ny, nz)
    a, neg = divmod(up_index(up), 2)
    b, c = [ax for ax in range(3) if ax != a]                    # the in-layer axes A and B, ascending
    na = n[a]
    offsets = disc(r2)

    def is_in(p):
        return all(0 <= p[ax] < n[ax] for ax in range(3)) and bool(inside[p[2], p[1], p[0]])

    def point(h, pb, pc):
        p = [0, 0, 0]
        p[a], p[b], p[c] = (na - 1 - h if neg else h), pb, pc
        return tuple(p)

    def linear(p):
        return p[0] + nx * (p[1] + ny * p[2])

    occupied = [h for h in range(na) if any(is_in(point(h, pb, pc)) for pc in range(n[c]) for pb in range(n[b]))]
    h0 = (occupied[0] if occupied else 0) if plate is None else int(plate)
    labels = np.zeros(inside.shape, dtype=np.uint32)
    rows = []
    for h in range(h0, na):
        layer = sorted((point(h, pb, pc) for pc in range(n[c]) for pb in range(n[b])), key=linear)
        for seed in layer:
            if not is_in(seed) or labels[seed[2], seed[1], seed[0]]:
                continue
            number = len(rows) + 1
            members, stack = [], [seed]
            labels[seed[2], seed[1], seed[0]] = number
            while stack:
                p = stack.pop()
                members.append(p)
                for ax in (b, c):
                    for d in (-1, 1):
                        q = list(p)
                        q[ax] += d
                        if is_in(q) and not labels[q[2], q[1], q[0]]:
                            labels[q[2], q[1], q[0]] = number
                            stack.append(tuple(q))
            supported, below = 0, set()
            for p in members:
                found = False
                if h > h0:
                    for du, dv in offsets:
                        q = list(point(h - 1, p[b] + du, p[c] + dv))
                        if is_in(q):
                            found = True
                            below.add(int(labels[q[2], q[1], q[0]]))
                supported += int(h == h0 or found)
            pa, pb_ = [p[b] for p in members], [p[c] for p in members]
            rows.append([h, min(linear(p) for p in members), len(members), supported, sum(pa), sum(pb_), min(pa), max(pa), min(pb_),
                         max(pb_), min(below) if below else 0, max(below) if below else 0])
    return _finish(rows, labels, inside, h0, (2 - a, neg))


# ---- form (b): layer-wise ---------------------------------------------------------------------------------------------------------
def _moved(layer, du, dv, fill):
    """out[p] = layer[p - (du, dv)], `fill` beyond the layer (any dtype)."""
    out = np.full_like(layer, fill)
    n0, n1 = layer.shape
    if abs(du) < n0 and abs(dv) < n1:
        s0, d0 = (slice(0, n0 - du), slice(du, n0)) if du >= 0 else (slice(-du, n0), slice(0, n0 + du))
        s1, d1 = (slice(0, n1 - dv), slice(dv, n1)) if dv >= 0 else (slice(-dv, n1), slice(0, n1 + dv))
        out[d0, d1] = layer[s0, s1]
    return out


def layer_components(layer):
    """The 4-connected components of a boolean layer: int64 labels 1.. in the order of their first point (row-major), 0 outside."""
    none = np.int64(layer.size + 1)
    lab = np.where(layer, np.arange(1, layer.size + 1, dtype=np.int64).reshape(layer.shape), none)
    while True:
        new = lab
        for du, dv in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            new = np.minimum(new, _moved(lab, du, dv, none))
        new = np.where(layer, new, none)
        # (pointer jumping: a point takes the label of the point its label names -- the same component, never a larger label)
        flat = np.append(new.reshape(-1), none)
        new = np.where(layer, np.minimum(new, flat[np.minimum(new, none) - 1].reshape(layer.shape)), none)
        if np.array_equal(new, lab):
            break
        lab = new
    roots = np.unique(lab[layer])
    out = np.zeros(layer.shape, dtype=np.int64)
    out[layer] = np.searchsorted(roots, lab[layer]) + 1
    return out, roots - 1                                        # the components' first points, as row-major indices


def layerwise(occ, up="+z", r2=1, plate=None):
    inside = np.asarray(occ) != 0
    nz, ny, nx = inside.shape
    a, neg = divmod(up_index(up), 2)
    npaxis = 2 - a                                               # occ is indexed [k, j, i]
    A = np.moveaxis(inside, npaxis, 0)                           # [h, B, A]
    if neg:
        A = A[::-1]
    nh, nb, na_ = A.shape
    filled = np.flatnonzero(A.reshape(nh, -1).any(axis=1))
    h0 = (int(filled[0]) if len(filled) else 0) if plate is None else int(plate)
    strides = [s for ax, s in enumerate((1, nx, nx * ny)) if ax != a]      # of A and B in the caller's linear index
    up_stride = (1, nx, nx * ny)[a]
    L = np.zeros(A.shape, dtype=np.int64)
    rows, count = [], 0
    cb, ca = np.meshgrid(np.arange(nb), np.arange(na_), indexing="ij")
    offsets = [(du, dv) for du, dv in disc(r2) if abs(du) < na_ and abs(dv) < nb]   # (a longer offset leaves the layer)
    for h in range(h0, nh):
        comp, first = layer_components(A[h])
        k = len(first)
        if k == 0:
            continue
        L[h] = np.where(comp > 0, comp + count, 0)
        idx = comp[A[h]] - 1
        cover = np.zeros_like(A[h])
        mn = np.full(k, np.iinfo(np.int64).max)
        mx = np.zeros(k, dtype=np.int64)
        if h > h0:
            for du, dv in offsets:
                # the label of the point at (A + du, B + dv) of the layer below, seen from this layer's point
                moved = _moved(L[h - 1], -dv, -du, 0)
                cover |= moved > 0
                here = moved[A[h]]
                np.minimum.at(mn, idx, np.where(here > 0, here, np.iinfo(np.int64).max))
                np.maximum.at(mx, idx, here)
        else:
            cover[:] = True
        mn[mx == 0] = 0
        pts = np.bincount(idx, minlength=k)
        table = np.zeros((k, 12), dtype=np.int64)
        table[:, LAYER] = h
        table[:, FIRST] = (first % na_) * strides[0] + (first // na_) * strides[1] + (nh - 1 - h if neg else h) * up_stride
        table[:, POINTS] = pts
        table[:, SUPPORTED] = np.bincount(idx, weights=cover[A[h]], minlength=k)
        table[:, SUM_A] = np.bincount(idx, weights=ca[A[h]], minlength=k)
        table[:, SUM_B] = np.bincount(idx, weights=cb[A[h]], minlength=k)
        for col, src, fn in ((MIN_A, ca, np.minimum), (MAX_A, ca, np.maximum), (MIN_B, cb, np.minimum), (MAX_B, cb, np.maximum)):
            acc = np.full(k, 1 << 40 if fn is np.minimum else -1, dtype=np.int64)
            fn.at(acc, idx, src[A[h]])
            table[:, col] = acc
        table[:, BELOW_MIN], table[:, BELOW_MAX] = mn, mx
        rows.append(table)
        count += k
    rows = np.concatenate(rows) if rows else np.zeros((0, 12), dtype=np.int64)
    labels = np.ascontiguousarray(np.moveaxis(L[::-1] if neg else L, 0, npaxis)).astype(np.uint32)
    return _finish(rows, labels, inside, h0, (npaxis, neg))


def solid(cc, words, origin, step, shape, level, max_dist=100.0, up="+z", r2=1, plate=None):
    """layerwise() of the solid d < level on the lattice, d the oracle's map_scene (mass_ref.lattice_inside)."""
    return layerwise(mass_ref.lattice_inside(cc, words, origin, step, shape, level, max_dist), up, r2, plate)


def roots(rows):
    """The island or base region every region grows from: one pass over the rows, which are sorted by layer."""
    root = np.zeros(len(rows) + 1, dtype=np.int64)
    for r in range(1, len(rows) + 1):
        below = int(rows[r - 1][BELOW_MIN])
        root[r] = root[below] if below else r
    return root[1:]


def same(x, y):
    """Two Results agree in every word."""
    return (x.counts == y.counts and np.array_equal(x.rows, y.rows) and np.array_equal(x.labels, y.labels) and
            np.array_equal(x.mask, y.mask) and np.array_equal(x.profile, y.profile))


# ---- the closed-form parts of the tests -------------------------------------------------------------------------------------------
def stalactites():
    """16 x 12 x 10 points (x, y, z): a 2 x 2 leg at x, y 1..2, z 0..7 under a slab x 1..14, y 1..10 at z 8, from which three
    posts hang: (6, 5) z 5..7, (10, 5) z 7, (13, 9) z 3..7.  Up +z every post starts in mid air: three islands of one point; the
    slab rests on the leg and on the three posts: the one merge.  Up -z everything grows from the slab."""
    occ = np.zeros((10, 12, 16), dtype=np.uint8)
    occ[0:8, 1:3, 1:3] = 1
    occ[8, 1:11, 1:15] = 1
    occ[5:8, 5, 6] = 1
    occ[7, 5, 10] = 1
    occ[3:8, 9, 13] = 1
    return occ


def sphere24():
    """The sphere of radius 1.5 on 24^3 points over [-2, 2]^3, indexed [k, j, i]."""
    x = -2.0 + 4.0 * np.arange(24) / 23.0
    zz, yy, xx = np.meshgrid(x, x, x, indexing="ij")
    return (xx * xx + yy * yy + zz * zz < 1.5 * 1.5).astype(np.uint8)


def checkerboard(shape=(6, 9, 11)):
    """(i + j + k) even on 11 x 9 x 6 points: every inside point is a region of its own."""
    k, j, i = np.indices(shape)
    return ((i + j + k) % 2 == 0).astype(np.uint8)
