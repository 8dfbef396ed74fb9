"""A numpy restatement of the surface-measure contract, for the tests.  counts(classes): pad with zeros,
per direction two shifted views of the padded array and a bincount of 8 a + b, the [0][0] row zeroed; measures(): binary64,
operation for operation as the contract writes them.  weights_quadrature(): the direction weights by a deterministic quadrature
of the 26 directions' Voronoi cells, independent of tools/surface_weights.py's closed form.  Written from the contract, not from
the kernel.  Test infrastructure only."""
import math

import numpy as np

CLASSES, DIRS, COUNTS = 8, 13, 840
DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1),
              (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1),
              (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1))
MEASURE_NAMES = ("area", "facet_area", "facet_pos_x", "facet_neg_x", "facet_pos_y", "facet_neg_y", "facet_pos_z", "facet_neg_z")
# axis, face diagonal, space diagonal: tools/surface_weights.py
WEIGHTS = (0.091555782409523431, 0.073961255752150262, 0.070391279564633452)


def pair_index(a, b, nu):
    return 8 + (8 * a + b) * 13 + nu


def classes_of(data):
    """min(byte, 7) of an array of a one-byte type, indexed [k, j, i]."""
    return np.minimum(np.ascontiguousarray(data).view(np.uint8), 7)


def counts(data):
    """The 840 words of rm_surface_classes for `data` (nz, ny, nx) of a one-byte type: uint64."""
    c = classes_of(data).astype(np.int64)
    out = np.zeros(COUNTS, dtype=np.uint64)
    out[:CLASSES] = np.bincount(c.reshape(-1), minlength=CLASSES).astype(np.uint64)
    p = np.pad(c, 1, constant_values=0)
    nz, ny, nx = p.shape

    def view(dx, dy, dz):
        """Two views of the padded lattice: the points p for which p + (dx, dy, dz) is in it too, and those p + (dx, dy, dz)."""
        def span(n, d):
            return (max(0, -d), n - max(0, d))
        (x0, x1), (y0, y1), (z0, z1) = span(nx, dx), span(ny, dy), span(nz, dz)
        return (slice(z0, z1), slice(y0, y1), slice(x0, x1)), (slice(z0 + dz, z1 + dz), slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))

    for nu, (dx, dy, dz) in enumerate(DIRECTIONS):
        first, second = view(dx, dy, dz)
        key = 8 * p[first] + p[second]
        table = np.bincount(key.reshape(-1), minlength=64).astype(np.uint64)
        table[0] = 0
        out[8 + np.arange(64) * 13 + nu] = table
    return out


def points(words):
    return np.asarray(words[:CLASSES], dtype=np.uint64)


def pairs(words):
    return np.asarray(words[8:], dtype=np.uint64).reshape(CLASSES, CLASSES, DIRS)


def measures(words, step, set_a, set_b):
    """rm_surface_measures for the class sets (iterables of classes): a dict MEASURE_NAMES -> float."""
    set_a, set_b = sorted(set(set_a)), sorted(set(set_b))
    assert set_a and set_b and not set(set_a) & set(set_b)
    P = pairs(words)
    st = [float(np.float32(s)) for s in step]
    fwd = [sum(int(P[a, b, nu]) for a in set_a for b in set_b) for nu in range(DIRS)]
    back = [sum(int(P[b, a, nu]) for a in set_a for b in set_b) for nu in range(DIRS)]
    out = {}
    facets = 0.0
    for ax, name in enumerate("xyz"):
        cell = st[(ax + 1) % 3] * st[(ax + 2) % 3]
        out["facet_pos_" + name] = cell * float(fwd[ax])
        out["facet_neg_" + name] = cell * float(back[ax])
        facets += out["facet_pos_" + name] + out["facet_neg_" + name]
    out["facet_area"] = facets
    if not (np.float32(step[0]) == np.float32(step[1]) == np.float32(step[2])):
        out["area"] = math.nan
        return out
    dV = st[0] * st[1] * st[2]
    total = 0.0
    for nu, d in enumerate(DIRECTIONS):
        v = [d[k] * st[k] for k in range(3)]
        kind = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        total += WEIGHTS[kind - 1] * float(fwd[nu] + back[nu]) / math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    out["area"] = 2.0 * dV * total
    return out


def ball(radius, centre_offset=(0.0, 0.0, 0.0), margin=2):
    """The occupancy (uint8, cubic) of a ball of `radius` index units whose centre lies `centre_offset` from the lattice's middle point."""
    n = 2 * (int(math.ceil(radius)) + margin) + 1
    mid = (n - 1) / 2.0
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    cx, cy, cz = (mid + o for o in centre_offset)
    return (((i - cx) ** 2 + (j - cy) ** 2 + (k - cz) ** 2) < radius * radius).astype(np.uint8)


def weights_quadrature(n):
    """The three weights by the midpoint rule on n latitudes x 2 n longitudes: each sample goes to the nearest of the 26 directions."""
    d = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)], dtype=np.float64)
    kind = (d * d).sum(axis=1).astype(np.int64)
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    h = math.pi / n
    ph = (np.arange(2 * n) + 0.5) * h
    w = np.zeros(4)
    for t in (np.arange(n) + 0.5) * h:
        u = np.stack([math.sin(t) * np.cos(ph), math.sin(t) * np.sin(ph), np.full_like(ph, math.cos(t))], axis=1)
        w += np.bincount(kind[np.argmax(u @ d.T, axis=1)], minlength=4) * (math.sin(t) * h * h)
    w /= 4.0 * math.pi
    return (w[1] / 3.0, w[2] / 6.0, w[3] / 4.0)
