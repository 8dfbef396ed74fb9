"""A numpy restatement of the overhang-and-support contract, for the tests, in two independent forms:
per_point(occ, ...) follows the definitions word for word -- per point a loop over the disc of the layer below, a walk up the
column to the first inside point, a walk down to the plate --; layerwise(occ, ...) turns the lattice so that the height is the first
axis and works on whole layers: shifted boolean arrays for the disc, the F recurrence top-down and the P recurrence bottom-up.
Both return (mask uint8 (nz, ny, nx), counts COUNT_NAMES -> int, profile uint32 (n_a, 4)).  Written from the contract, not from
the kernels.  Test infrastructure only."""
import numpy as np

import mass_ref

UPS = ("+x", "-x", "+y", "-y", "+z", "-z")                       # RM_UP_POS_X .. RM_UP_NEG_Z
COUNT_NAMES = ("points", "plate", "base", "overhang", "support_on_plate", "support_on_part", "runs", "landings")
OUTSIDE, INSIDE, OVERHANG, ON_PLATE, ON_PART = range(5)


def up_index(up):
    return UPS.index(up) if isinstance(up, str) else int(up)


def disc(r2):
    """The offsets (du, dv) with du^2 + dv^2 <= r2."""
    r = int(np.floor(np.sqrt(r2)))
    return [(du, dv) for du in range(-r, r + 1) for dv in range(-r, r + 1) if du * du + dv * dv <= r2]


def _counts(mask_h, inside_h, h0):
    """counts and profile from the mask with the height as its first axis."""
    nh = mask_h.shape[0]
    profile = np.zeros((nh, 4), dtype=np.uint32)
    for h in range(nh):
        profile[h] = [np.count_nonzero(inside_h[h]), np.count_nonzero(mask_h[h] == OVERHANG), np.count_nonzero(mask_h[h] == ON_PLATE),
                      np.count_nonzero(mask_h[h] == ON_PART)]
    sup = mask_h >= ON_PLATE
    runs = sum(np.count_nonzero(sup[h] & (mask_h[h + 1] == OVERHANG)) for h in range(nh - 1))
    landings = sum(np.count_nonzero(sup[h] & inside_h[h - 1]) for h in range(h0 + 1, nh))
    c = {"points": int(profile[:, 0].sum()), "plate": int(h0), "base": int(profile[h0, 0]), "overhang": int(profile[:, 1].sum()),
         "support_on_plate": int(profile[:, 2].sum()), "support_on_part": int(profile[:, 3].sum()), "runs": int(runs),
         "landings": int(landings)}
    return c, profile


# ---- form (a): per point ----------------------------------------------------------------------------------------------------------
def per_point(occ, up="+z", r2=1, plate=None):
    inside = np.asarray(occ) != 0
    nz, ny, nx = inside.shape
    n = (nx, ny, nz)
    a, neg = divmod(up_index(up), 2)
    b, c = [ax for ax in range(3) if ax != a]
    na = n[a]
    offsets = disc(r2)

    def is_in(p):
        return all(0 <= p[ax] < n[ax] for ax in range(3)) and bool(inside[p[2], p[1], p[0]])

    def height(p):
        return na - 1 - p[a] if neg else p[a]

    def at_height(p, h):
        q = list(p)
        q[a] = na - 1 - h if neg else h
        return tuple(q)

    points = [(i, j, k) for k in range(nz) for j in range(ny) for i in range(nx)]
    heights = [height(p) for p in points if is_in(p)]
    h0 = (min(heights) if heights else 0) if plate is None else int(plate)

    def overhang(p):
        h = height(p)
        if not is_in(p) or h <= h0:
            return False
        for du, dv in offsets:
            q = list(at_height(p, h - 1))
            q[b] += du
            q[c] += dv
            if is_in(q):
                return False
        return True

    mask = np.zeros(inside.shape, dtype=np.uint8)
    for p in points:
        h = height(p)
        if is_in(p):
            mask[p[2], p[1], p[0]] = OVERHANG if overhang(p) else INSIDE
            continue
        if h < h0:
            continue
        above = next((at_height(p, g) for g in range(h + 1, na) if is_in(at_height(p, g))), None)
        if above is None or not overhang(above):
            continue
        on_plate = not any(is_in(at_height(p, g)) for g in range(h0, h))
        mask[p[2], p[1], p[0]] = ON_PLATE if on_plate else ON_PART
    # the counts, per point again
    runs = landings = 0
    for p in points:
        h = height(p)
        if mask[p[2], p[1], p[0]] < ON_PLATE:
            continue
        if h + 1 < na:
            q = at_height(p, h + 1)
            runs += int(mask[q[2], q[1], q[0]] == OVERHANG)
        if h > h0:
            landings += int(is_in(at_height(p, h - 1)))
    npaxis = 2 - a
    mask_h = np.moveaxis(mask, npaxis, 0)[::-1] if neg else np.moveaxis(mask, npaxis, 0)
    inside_h = np.moveaxis(inside, npaxis, 0)[::-1] if neg else np.moveaxis(inside, npaxis, 0)
    counts, profile = _counts(mask_h, inside_h, h0)
    assert counts["runs"] == runs and counts["landings"] == landings
    return mask, counts, profile


# ---- form (b): layer-wise ---------------------------------------------------------------------------------------------------------
def _shifted(layer, du, dv):
    """out[p] = layer[p - (du, dv)] (False beyond the layer): the layer moved by (du, dv) along its two axes."""
    out = np.zeros_like(layer)
    n0, n1 = layer.shape
    s0, d0 = (slice(0, n0 - du), slice(du, n0)) if du >= 0 else (slice(-du, n0), slice(0, n0 + du))
    s1, d1 = (slice(0, n1 - dv), slice(dv, n1)) if dv >= 0 else (slice(-dv, n1), slice(0, n1 + dv))
    if abs(du) < n0 and abs(dv) < n1:
        out[d0, d1] = layer[s0, s1]
    return out


def dilated(layer, r2):
    """The points of a layer within the disc of some True point: the OR of the layer moved by every offset of the disc.  (The
    offsets of one du form a run of dv: moved by du, then a window of 2 w + 1 points along the other axis, by a running sum.)"""
    out = np.zeros_like(layer)
    r = int(np.floor(np.sqrt(r2)))
    n1 = layer.shape[1]
    for du in range(-r, r + 1):
        w = 0
        while (w + 1) ** 2 + du * du <= r2:
            w += 1
        moved = _shifted(layer, du, 0)
        run = np.concatenate([np.zeros((moved.shape[0], w + 1), dtype=np.int64), np.cumsum(moved, axis=1, dtype=np.int64),
                              np.repeat(moved.sum(axis=1, dtype=np.int64)[:, None], w, axis=1)], axis=1)
        out |= (run[:, 2 * w + 1:2 * w + 1 + n1] - run[:, 0:n1]) > 0
    return out


def layerwise(occ, up="+z", r2=1, plate=None):
    inside = np.asarray(occ) != 0
    a, neg = divmod(up_index(up), 2)
    npaxis = 2 - a                                               # occ is indexed [k, j, i]
    A = np.moveaxis(inside, npaxis, 0)
    if neg:
        A = A[::-1]
    nh = A.shape[0]
    filled = np.flatnonzero(A.reshape(nh, -1).any(axis=1))
    h0 = (int(filled[0]) if len(filled) else 0) if plate is None else int(plate)
    ov = np.zeros_like(A)
    for h in range(h0 + 1, nh):
        ov[h] = A[h] & ~dilated(A[h - 1], r2)
    sup = np.zeros_like(A)
    F = np.zeros_like(A[0])
    for h in range(nh - 1, h0 - 1, -1):
        sup[h] = F & ~A[h]
        F = (F & ~A[h]) | ov[h]
    plt = np.zeros_like(A)
    P = np.ones_like(A[0])
    for h in range(h0, nh):
        plt[h] = sup[h] & P
        P = P & ~A[h]
    mask_h = np.where(A, np.where(ov, OVERHANG, INSIDE), np.where(sup, np.where(plt, ON_PLATE, ON_PART), OUTSIDE)).astype(np.uint8)
    counts, profile = _counts(mask_h, A, h0)
    # RUNS and LANDINGS by the recurrences' own popcounts
    assert counts["runs"] == sum(np.count_nonzero(ov[h + 1] & ~A[h]) for h in range(h0, nh - 1))
    assert counts["landings"] == sum(np.count_nonzero(sup[h] & A[h - 1]) for h in range(h0 + 1, nh))
    mask = np.moveaxis(mask_h[::-1] if neg else mask_h, 0, npaxis)
    return np.ascontiguousarray(mask), counts, profile


def solid(cc, words, origin, step, shape, level, max_dist=100.0, up="+z", r2=1, plate=None):
    """layerwise() of the solid d < level on the lattice, d the oracle's map_scene (mass_ref.lattice_inside)."""
    return layerwise(mass_ref.lattice_inside(cc, words, origin, step, shape, level, max_dist), up, r2, plate)


# ---- the closed-form parts of the tests -------------------------------------------------------------------------------------------
def table():
    """12 x 10 x 9 points: a 2 x 2 leg at i 5..6, j 4..5, k 0..5 under a 10 x 8 top at i 1..10, j 1..8, k 6..7."""
    occ = np.zeros((9, 10, 12), dtype=np.uint8)
    occ[0:6, 4:6, 5:7] = 1
    occ[6:8, 1:9, 1:11] = 1
    return occ


TABLE_OVERHANG = {0: 76, 1: 68, 2: 64, 4: 56}                  # r2 -> overhang points, up +z


def shelf():
    """16 x 12 x 12 points: a base slab over the whole layer at k 1..2, a 2 x 2 post at i 3..4, j 3..4, k 3..7, and a shelf
    i 3..11, j 2..8 at k 8.  Up +z, r2 = 0: the shelf's 9 x 7 points overhang but for the 4 over the post, every support column
    stands on the slab: 59 runs of 5 points (k 3..7), 59 landings, none on the plate."""
    occ = np.zeros((12, 12, 16), dtype=np.uint8)
    occ[1:3, :, :] = 1
    occ[3:8, 3:5, 3:5] = 1
    occ[8, 2:9, 3:12] = 1
    return occ
