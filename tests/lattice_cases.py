"""Lattices and rays the lattice-draw tests share, in numpy alone: the contents the issue names, random rays
from outside and inside a lattice's box, and the degenerate rays -- axis-parallel, in a plane between cells, through lattice
vertices, from a face or from inside a full cell, pointing away, a zero direction, NaN and infinite components, an origin
near 1e8 where planes collapse to one t, direction components of 1e-30 and denormal."""
import numpy as np

F = np.float32
ORIGIN = np.asarray([-1.25, 0.5, 2.0], dtype=F)
STEP = np.asarray([0.25, 0.5, 0.375], dtype=F)
CONTENTS = ("empty", "full", "corners", "random", "sparse", "one_per_brick", "hollow_brick")
PALETTE = [[0.4, 0.7, 0.1], [0.9, 0.1, 0.1], [0.1, 0.2, 0.9], [0.8, 0.8, 0.2], [0.5, 0.5, 0.5]]


def contents(shape, kind, seed=0):
    """uint8 (nz, ny, nx) for a shape (nx, ny, nz)."""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    c = np.zeros((nz, ny, nx), dtype=np.uint8)
    if kind == "full":
        c[:] = rng.integers(1, 256, size=c.shape)
    elif kind == "corners":
        c[0, 0, 0], c[-1, -1, -1], c[0, -1, 0] = 1, 255, 4
    elif kind == "random":
        c[:] = rng.integers(0, 256, size=c.shape) * (rng.random(c.shape) < 0.5)
    elif kind == "sparse":
        c[:] = rng.integers(1, 256, size=c.shape) * (rng.random(c.shape) < 0.1)
    elif kind == "one_per_brick":
        for k in range(0, nz, 8):
            for j in range(0, ny, 8):
                for i in range(0, nx, 8):
                    c[min(nz - 1, k + rng.integers(8)), min(ny - 1, j + rng.integers(8)), min(nx - 1, i + rng.integers(8))] = 1 + (i + j + k) % 7
    elif kind == "hollow_brick":
        c[:] = 3
        c[8:16, 8:16, 8:16] = 0
    else:
        assert kind == "empty"
    return c


def box(shape, origin=ORIGIN, step=STEP):
    o, s = np.asarray(origin, dtype=np.float64), np.asarray(step, dtype=np.float64)
    return o - 0.5 * s, o + (np.asarray(shape) - 0.5) * s


def random_rays(shape, n, seed=1, origin=ORIGIN, step=STEP):
    """n rays: a third from inside the box, the rest from around it; two in three aim at a point of the box."""
    rng = np.random.default_rng(seed)
    lo, hi = box(shape, origin, step)
    O = lo + (hi - lo) * (3.0 * rng.random((n, 3)) - 1.0)
    inside = np.arange(n) % 3 == 0
    O[inside] = (lo + (hi - lo) * rng.random((n, 3)))[inside]
    D = rng.standard_normal((n, 3))
    aimed = (np.arange(n) // 3) % 3 != 0
    D[aimed] = ((lo + (hi - lo) * rng.random((n, 3))) - O)[aimed]
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    return np.concatenate([O, D], axis=1).astype(F)


def degenerate_rays(shape, seed=2, origin=ORIGIN, step=STEP):
    """The issue's degenerate set for a lattice, as (n, 6) float32."""
    rng = np.random.default_rng(seed)
    o, s, n = np.asarray(origin, dtype=F), np.asarray(step, dtype=F), np.asarray(shape)
    lo, hi = box(shape, origin, step)
    centre = lambda c: (o + np.asarray(c, dtype=F) * s).astype(F)  # noqa: E731  (the centre of a cell: exact for these lattices)
    rays = []
    add = lambda O, D: rays.append(np.concatenate([np.asarray(O, dtype=F), np.asarray(D, dtype=F)]))  # noqa: E731
    for a in range(3):
        for sign in (1.0, -1.0):
            d = np.zeros(3); d[a] = sign
            for _ in range(6):                                   # axis-parallel, through cell centres and anywhere
                c = rng.integers(0, n)
                start = centre(c); start[a] = (lo[a] - 1.0) if sign > 0 else (hi[a] + 1.0)
                add(start, d)
                add(lo + (hi - lo) * rng.random(3), d)
                add(start, -d)                                   # pointing away
            for _ in range(6):                                   # in the plane between cells m - 1 and m of axis a
                m = rng.integers(0, n[a] + 1)
                start = (lo + (hi - lo) * (2.0 * rng.random(3) - 0.5)).astype(F)
                start[a] = o[a] + (F(m) - F(0.5)) * s[a]
                d2 = rng.standard_normal(3); d2[a] = 0.0
                add(start, d2)
                d2[(a + 1) % 3] = 0.0                            # ... and along an edge line
                add(start, d2 * sign)
    for sx in (1, -1):                                           # the diagonal through lattice vertices: three-way ties
        for sy in (1, -1):
            for sz in (1, -1):
                sg = np.asarray([sx, sy, sz], dtype=F)
                for k in (1.5, 0.5, 2.5):
                    corner = np.where(sg > 0, -0.5, n - 0.5).astype(F)
                    add(o + (corner - sg * F(k)) * s, sg * s)
                add(centre(n // 2) + F(0.5) * s, sg * s)         # from a vertex inside
    for _ in range(12):                                          # an origin on a window face, and inside a cell
        a = rng.integers(3)
        start = (lo + (hi - lo) * rng.random(3)).astype(F)
        start[a] = (lo if rng.random() < 0.5 else hi)[a]
        add(start, rng.standard_normal(3))
        add(centre(rng.integers(0, n)), rng.standard_normal(3))
        add(centre(rng.integers(0, n)), np.zeros(3))             # a zero direction
    add(lo - 1.0, np.zeros(3))
    for bad in (np.nan, np.inf, -np.inf):                        # NaN / inf components
        for a in range(3):
            start, d = centre(n // 2), np.asarray([0.3, -0.5, 0.8]); start[a] = bad
            add(start, d)
            start, d = (lo - 1.0).astype(F), np.asarray([0.5, 0.6, 0.7]); d[a] = bad
            add(start, d)
    for a in range(3):                                           # |O| ~ 1e8: the planes of an axis collapse to one t
        for sign in (1.0, -1.0):
            start = centre(n // 2); start[a] = sign * 1e8
            d = 0.01 * rng.standard_normal(3); d[a] = -sign
            add(start, d)
            add(start + F(3.0), d)
            d = np.zeros(3); d[a] = -sign
            add(start, d)
    tiny = (1e-30, -1e-30, float(np.finfo(F).smallest_subnormal), -float(np.finfo(F).smallest_subnormal), 1e-38, 3e-39)
    for t in tiny:                                               # direction components of 1e-30 and denormal
        for a in range(3):
            d = np.full(3, t); d[a] = 1.0
            add((lo - 0.25).astype(F), d)
            add(centre(n // 2) + F(0.125) * s, d)
            d = np.full(3, t)
            add(centre(n // 3), d)
            d = rng.standard_normal(3); d[a] = t
            add((lo + (hi - lo) * rng.random(3)).astype(F), d)
    return np.asarray(rays, dtype=F)


def windows(shape, seed=3):
    """A few windows of a lattice: a slab, a corner octant, a single cell, one interior box."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    lo = [int(rng.integers(0, v - 1)) for v in shape]
    hi = [int(rng.integers(l + 1, v + 1)) for l, v in zip(lo, shape)]
    return [(0, 0, nz // 2, nx, ny, nz), (0, 0, 0, (nx + 1) // 2, (ny + 1) // 2, (nz + 1) // 2), (nx - 1, ny - 1, 0, nx, ny, 1), tuple(lo + hi)]
