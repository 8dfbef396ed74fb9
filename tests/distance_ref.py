"""A numpy restatement of the distance-transform contract, for the tests, in two independent forms:
brute(occ) takes every point against every point of the other class (and the layer rule in closed form), in chunks; separable(occ)
makes three axis passes, each the full min_q g(q) + (p - q)^2 by broadcasting -- no window, no early exit.  features() follows the
definitions of core, opened, thin and narrow word for word.  Written from the contract, not from the kernels.  Test
infrastructure only."""
import numpy as np

import mass_ref

INSIDE_BIT = 0x80000000
NONE = 0x7FFFFFFF
NO_INDEX = 0xFFFFFFFF
COUNT_NAMES = ("points", "max_inside", "argmax_inside", "max_outside", "argmax_outside")
FEATURE_NAMES = ("core", "thin", "gap_core", "narrow")
BIG = np.int64(1) << 40


def layer_bound(shape):
    """int64 (nz, ny, nx): the squared distance of every point to the nearest point of the surrounding layer,
    min(i + 1, nx - i, j + 1, ny - j, k + 1, nz - k)^2."""
    nz, ny, nx = shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    m = np.minimum.reduce([i + 1, nx - i, j + 1, ny - j, k + 1, nz - k]).astype(np.int64)
    return m * m


def nearest_brute(targets, sources):
    """int64 per target row: the smallest squared distance to a source row (BIG for no sources).  targets, sources: (n, 3) int64."""
    out = np.full(len(targets), BIG, dtype=np.int64)
    if len(sources) == 0:
        return out
    chunk = max(1, (1 << 21) // len(sources))                  # about 50 MB of differences at a time
    for a in range(0, len(targets), chunk):
        d = targets[a:a + chunk, None, :] - sources[None, :, :]
        out[a:a + chunk] = (d * d).sum(axis=2).min(axis=1)
    return out


def brute(occ):
    """occ: (nz, ny, nx), nonzero = inside.  uint32 (nz, ny, nx): the distance volume."""
    inside = np.asarray(occ) != 0
    coords = np.stack(np.nonzero(np.ones(inside.shape, dtype=bool)), axis=1).astype(np.int64).reshape(inside.shape + (3,))
    pin, pout = coords[inside], coords[~inside]
    d = np.zeros(inside.shape, dtype=np.int64)
    d[inside] = np.minimum(nearest_brute(pin, pout), layer_bound(inside.shape)[inside])
    d[~inside] = np.minimum(nearest_brute(pout, pin), NONE)
    return (d.astype(np.uint32) | np.where(inside, np.uint32(INSIDE_BIT), np.uint32(0))).astype(np.uint32)


def axis_pass(g, axis, layer):
    """f(p) = min_q g(q) + (p - q)^2 along `axis` (int64, BIG = no value), with g = 0 at q = -1 and q = n when `layer`."""
    g = np.moveaxis(g, axis, -1)
    n = g.shape[-1]
    if layer:
        g = np.concatenate([np.zeros(g.shape[:-1] + (1,), dtype=np.int64), g, np.zeros(g.shape[:-1] + (1,), dtype=np.int64)], axis=-1)
        q = np.arange(-1, n + 1, dtype=np.int64)
    else:
        q = np.arange(n, dtype=np.int64)
    p = np.arange(n, dtype=np.int64)
    off = (p[:, None] - q[None, :]) ** 2                       # (n, len q)
    f = np.empty(g.shape[:-1] + (n,), dtype=np.int64)
    flat_g, flat_f = g.reshape(-1, g.shape[-1]), f.reshape(-1, n)
    rows = max(1, (1 << 22) // (n * len(q)))
    for a in range(0, len(flat_g), rows):
        flat_f[a:a + rows] = (flat_g[a:a + rows, None, :] + off[None, :, :]).min(axis=2)
    return np.moveaxis(np.minimum(f, BIG), -1, axis)


def transform(sources, layer):
    """int64: the squared distance of every point to the nearest True point of `sources` (BIG for none), the layer's points
    counting as sources when `layer`."""
    g = np.where(sources, np.int64(0), BIG)
    for axis in (2, 1, 0):
        g = axis_pass(g, axis, layer)
    return g


def separable(occ):
    """The distance volume of brute(), by three axis passes per class."""
    inside = np.asarray(occ) != 0
    d = np.where(inside, transform(~inside, True), np.minimum(transform(inside, False), NONE))
    return (d.astype(np.uint32) | np.where(inside, np.uint32(INSIDE_BIT), np.uint32(0))).astype(np.uint32)


def counts(volume):
    """The five counts of a distance volume (COUNT_NAMES -> int)."""
    v = np.asarray(volume, dtype=np.uint32).ravel()
    inside = (v & INSIDE_BIT) != 0
    d = (v & NONE).astype(np.int64)
    out = {"points": int(np.count_nonzero(inside))}
    for name, sel in (("inside", inside), ("outside", ~inside)):
        if sel.any():
            m = int(d[sel].max())
            out["max_" + name], out["arg" + "max_" + name] = m, int(np.flatnonzero(sel & (d == m))[0])
        else:
            out["max_" + name], out["arg" + "max_" + name] = 0, NO_INDEX
    return out


def opened_complement(cls, d2, r2, distance=None):
    """(core, far): core = the points of `cls` with d2 > r2; far = the points of `cls` farther than r2 from every core point."""
    core = cls & (d2 > r2)
    dist = (distance or (lambda s: transform(s, False)))(core)
    return core, cls & ~(dist <= r2)


def features(occ, r2_wall=None, r2_gap=None, volume=None):
    """(mask uint8 (nz, ny, nx), counts FEATURE_NAMES -> int) from the definitions; None skips a half."""
    inside = np.asarray(occ) != 0
    v = separable(occ) if volume is None else np.asarray(volume, dtype=np.uint32)
    d2 = (v & NONE).astype(np.int64)
    mask = inside.astype(np.uint8)
    c = dict.fromkeys(FEATURE_NAMES, 0)
    if r2_wall is not None:
        core, thin = opened_complement(inside, d2, r2_wall)
        mask[thin] = 2
        c["core"], c["thin"] = int(np.count_nonzero(core)), int(np.count_nonzero(thin))
    if r2_gap is not None:
        core, narrow = opened_complement(~inside, d2, r2_gap)
        mask[narrow] = 3
        c["gap_core"], c["narrow"] = int(np.count_nonzero(core)), int(np.count_nonzero(narrow))
    return mask, c


def solid(cc, words, origin, step, shape, level, max_dist=100.0):
    """separable() of the solid d < level on the lattice, d the oracle's map_scene (mass_ref.lattice_inside)."""
    return separable(mass_ref.lattice_inside(cc, words, origin, step, shape, level, max_dist))
