"""A numpy restatement of the mass-property contract, for the tests: the sixteen integer moments of the
occupancy lattice {d < level} from the oracle's lattice distances -- no bricks, no skipping -- ; a model of the brick classes
(kept / inside / outside) built on tests/sparse_ref.py's model of the skipping rule, which predicts rm_mass_moments' statistics;
and rm_mass_from_moments in exact rational arithmetic.  Test infrastructure only."""
from fractions import Fraction

import numpy as np

import mesh_ref
import sparse_ref
from oracle import rm_oracle_np as onp

F = np.float32
BRICK = 8
NO_MIN = 0xFFFFFFFF
(COUNT, X, Y, Z, XX, YY, ZZ, XY, YZ, XZ, MIN_X, MIN_Y, MIN_Z, MAX_X, MAX_Y, MAX_Z) = range(16)


# ---- moments --------------------------------------------------------------------------------------------------------------------
def moments_of_indices(i, j, k):
    """The 16 moments (Python ints) of the index set {(i[n], j[n], k[n])}."""
    i, j, k = (np.asarray(a, dtype=np.int64).ravel() for a in (i, j, k))      # indices < 2^12 and < 2^36 of them: int64 sums are exact
    if len(i) == 0:
        return [0] * 10 + [NO_MIN] * 3 + [0] * 3
    s = lambda a: int(a.sum(dtype=np.int64))  # noqa: E731
    return [len(i), s(i), s(j), s(k), s(i * i), s(j * j), s(k * k), s(i * j), s(j * k), s(i * k),
            int(i.min()), int(j.min()), int(k.min()), int(i.max()), int(j.max()), int(k.max())]


def moments_of_inside(inside, first=(0, 0, 0)):
    """inside: (nz, ny, nx) bool.  The moments of its True points, their indices counted from `first` = (i0, j0, k0)."""
    k, j, i = np.nonzero(np.asarray(inside, dtype=bool))
    return moments_of_indices(i + first[0], j + first[1], k + first[2])


def lattice_inside(cc, words, origin, step, shape, level, max_dist=100.0, first=(0, 0, 0), count=None):
    """(nz, ny, nx) bool: d < level at the points [first, first + count) of the lattice (all of it by default), d the oracle's
    map_scene at the coordinates the FULL lattice gives those points."""
    count = tuple(shape[a] - first[a] for a in range(3)) if count is None else count
    xs, ys, zs = (c[first[a]:first[a] + count[a]] for a, c in enumerate(mesh_ref.axis_coords(origin, step, shape)))
    z, y, x = np.meshgrid(zs, ys, xs, indexing="ij")
    with np.errstate(all="ignore"):
        if cc == 0:
            d = np.full(x.size, F(max_dist), dtype=F)
        else:
            d = np.asarray(onp.map_scene(cc, words, F(max_dist), x.ravel(), y.ravel(), z.ravel()), dtype=F)
        return (d < F(level)).reshape(count[2], count[1], count[0])           # NaN: outside


def lattice_moments(cc, words, origin, step, shape, level, max_dist=100.0):
    return moments_of_inside(lattice_inside(cc, words, origin, step, shape, level, max_dist))


def box_moments(lo, hi):
    """The moments of the index box [lo, hi) per axis, in closed form (Python ints of any size)."""
    n = [hi[a] - lo[a] for a in range(3)]
    if min(n) <= 0:
        return [0] * 10 + [NO_MIN] * 3 + [0] * 3
    s1 = [(lo[a] + hi[a] - 1) * n[a] // 2 for a in range(3)]
    sq = lambda m: (m - 1) * m * (2 * m - 1) // 6  # noqa: E731    sum of i^2 over [0, m)
    s2 = [sq(hi[a]) - sq(lo[a]) for a in range(3)]
    N = n[0] * n[1] * n[2]
    return [N, s1[0] * n[1] * n[2], s1[1] * n[0] * n[2], s1[2] * n[0] * n[1], s2[0] * n[1] * n[2], s2[1] * n[0] * n[2], s2[2] * n[0] * n[1],
            s1[0] * s1[1] * n[2], s1[1] * s1[2] * n[0], s1[0] * s1[2] * n[1], lo[0], lo[1], lo[2], hi[0] - 1, hi[1] - 1, hi[2] - 1]


# ---- the brick classes ----------------------------------------------------------------------------------------------------------
def class_model(cc, words, origin, step, shape, level, L, E, max_dist=100.0):
    """keep, inside: (bz, by, bx) bool; stats: what rm_mass_moments reports (without scratch_bytes).  keep is sparse_ref.brick_model's;
    a cleared brick is inside iff its probe value (the same probe) is < level; a kept brick is evaluated at its OWN points,
    min(8, n - i0) per axis."""
    keep, _ = sparse_ref.brick_model(cc, words, origin, step, shape, level, L, E, max_dist)
    cx, cy, cz = (sparse_ref._axis_tiles(origin[a], step[a], shape[a])[1] for a in range(3))
    pz, py, px = np.meshgrid(cz, cy, cx, indexing="ij")
    with np.errstate(all="ignore"):
        if cc == 0:
            v = np.full(px.shape, F(max_dist), dtype=F)
        else:
            v = np.asarray(onp.map_scene(cc, words, F(max_dist), px.ravel(), py.ravel(), pz.ravel()), dtype=F).reshape(px.shape)
        inside = ~keep & (v < F(level))
    own = [np.minimum(BRICK, shape[a] - np.arange(0, shape[a], BRICK)).astype(np.int64) for a in range(3)]
    points = own[2][:, None, None] * own[1][None, :, None] * own[0][None, None, :]
    stats = {"bricks": int(keep.size), "bricks_kept": int(np.count_nonzero(keep)), "bricks_inside": int(np.count_nonzero(inside)),
             "evaluations": int(keep.size + points[keep].sum())}
    return keep, inside, stats


def own_points_mixed(inside_points):
    """inside_points: (nz, ny, nx) bool.  (bz, by, bx) bool: the brick's OWN points lie on both sides; and (bz, by, bx) bool: all of
    them are inside."""
    nz, ny, nx = inside_points.shape
    bz, by, bx = ((n + BRICK - 1) // BRICK for n in (nz, ny, nx))
    mixed, full = np.zeros((bz, by, bx), dtype=bool), np.zeros((bz, by, bx), dtype=bool)
    for k in range(bz):
        for j in range(by):
            for i in range(bx):
                t = inside_points[k * BRICK:(k + 1) * BRICK, j * BRICK:(j + 1) * BRICK, i * BRICK:(i + 1) * BRICK]
                full[k, j, i] = t.all()
                mixed[k, j, i] = t.any() and not full[k, j, i]
    return mixed, full


# ---- rm_mass_from_moments, exactly ------------------------------------------------------------------------------------------------
def from_moments(m, origin, step, density=1.0):
    """The 17 properties (floats, RM_MASS_* order) of rm_mass_from_moments, every operation exact (Python int and Fraction) and
    one rounding to binary64 at the end."""
    m = [int(x) for x in m]
    o = [Fraction(float(F(x))) for x in origin]
    s = [Fraction(float(F(x))) for x in step]
    N = m[COUNT]
    if N == 0:
        return [0.0] * 11 + [float("inf")] * 3 + [float("-inf")] * 3
    dV = s[0] * s[1] * s[2]
    volume = N * dV
    mass = Fraction(float(density)) * volume
    S = m[X:Z + 1]
    c = [o[a] + s[a] * Fraction(S[a], N) for a in range(3)]
    second = {(0, 0): m[XX], (1, 1): m[YY], (2, 2): m[ZZ], (0, 1): m[XY], (1, 2): m[YZ], (0, 2): m[XZ]}
    mu = {}
    for (a, b), Sab in second.items():
        D = N * Sab - S[a] * S[b]
        mu[a, b] = s[a] * s[b] * Fraction(D, N * N) + (s[a] * s[a] / 12 if a == b else 0)
    out = [volume, mass] + c + [mass * (mu[1, 1] + mu[2, 2]), mass * (mu[0, 0] + mu[2, 2]), mass * (mu[0, 0] + mu[1, 1]),
                                -mass * mu[0, 1], -mass * mu[1, 2], -mass * mu[0, 2]]
    out += [o[a] + m[MIN_X + a] * s[a] for a in range(3)] + [o[a] + m[MAX_X + a] * s[a] for a in range(3)]
    return [float(x) for x in out]


def tolerances(expected, origin, step, shape):
    """Per entry: 1e-12 |expected|, and for centroid and box entries 1e-12 (|o_a| + n_a |s_a|): fewer than 50 binary64 roundings of
    1.1e-16 each, and no cancellation because the numerators are exact integers."""
    tol = [1e-12 * abs(x) if np.isfinite(x) else 0.0 for x in expected]
    for a in range(3):
        scale = 1e-12 * (abs(float(F(origin[a]))) + shape[a] * abs(float(F(step[a]))))
        for e in (2 + a, 11 + a, 14 + a):
            tol[e] = scale
    return tol
