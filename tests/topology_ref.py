"""A numpy restatement of the solid-topology contract, for the tests: bodies (6-adjacency) and voids
(26-adjacency) of an occupancy lattice by minimum propagation over shifted arrays with pointer jumping, the exterior by padding
with one outside layer, canonical numbers by smallest linear index, the sixteen moments per component through
mass_ref.moments_of_indices, and V, E, F, K from products of shifted arrays.  Written from the contract, not from the kernels:
no bricks, no union-find.  Test infrastructure only."""
import itertools

import numpy as np

import mass_ref

CAVITY_BIT = 0x80000000
EXTERIOR = 0xFFFFFFFF
COUNT_NAMES = ("bodies", "cavities", "points", "edges", "faces", "cells", "euler", "tunnels", "exterior_points")
FACES6 = [(0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)]                      # (dk, dj, di)
ALL26 = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]


def components(mask, offsets):
    """mask: (nz, ny, nx) bool.  int64 (nz, ny, nx): for every True point the smallest linear index (i + nx (j + ny k)) of its
    connected component under the neighbourhood `offsets`; -1 elsewhere."""
    mask = np.asarray(mask, dtype=bool)
    nz, ny, nx = mask.shape
    big = np.int64(mask.size)
    idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    lab = np.where(mask, idx, big)
    flat_mask = mask.ravel()
    while True:
        pad = np.pad(lab, 1, constant_values=big)
        m = lab.copy()
        for dk, dj, di in offsets:
            np.minimum(m, pad[1 + dk:1 + dk + nz, 1 + dj:1 + dj + ny, 1 + di:1 + di + nx], out=m)
        m = np.where(mask, m, big).ravel()
        # pointer jumping: a label is a point of the same component; take that point's label until nothing moves
        while True:
            nxt = m.copy()
            nxt[flat_mask] = m[m[flat_mask]]
            if np.array_equal(nxt, m):
                break
            m = nxt
        m = m.reshape(mask.shape)
        if np.array_equal(m, lab):
            break
        lab = m
    return np.where(mask, lab, -1)


def number(labels_of_points):
    """Canonical numbers: the rank of each point's label among the distinct labels, ascending.  (numbers, distinct labels)."""
    distinct = np.unique(labels_of_points)
    return np.searchsorted(distinct, labels_of_points), distinct


def topology(inside):
    """inside: (nz, ny, nx) bool.  A dict: counts (COUNT_NAMES -> int), body_rows and cavity_rows (lists of 16 ints each, in body
    and cavity order), labels (uint32 (nz, ny, nx))."""
    inside = np.asarray(inside, dtype=bool)
    nz, ny, nx = inside.shape
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    labels = np.full(inside.shape, EXTERIOR, dtype=np.uint32)
    # bodies
    body_lab = components(inside, FACES6)
    body_rows = []
    if inside.any():
        num, distinct = number(body_lab[inside])
        labels[inside] = num.astype(np.uint32)
        order = np.argsort(num, kind="stable")
        bounds = np.searchsorted(num[order], np.arange(len(distinct) + 1))
        pi, pj, pk = ii[inside][order], jj[inside][order], kk[inside][order]
        body_rows = [mass_ref.moments_of_indices(pi[a:b], pj[a:b], pk[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    # voids: the lattice surrounded by one layer of outside points; the void of that layer is the exterior
    outside_p = np.pad(~inside, 1, constant_values=True)
    void_lab = components(outside_p, ALL26)
    exterior_p = void_lab == void_lab[0, 0, 0]
    cavity = (~inside) & ~exterior_p[1:-1, 1:-1, 1:-1]
    exterior_points = int(np.count_nonzero((~inside) & exterior_p[1:-1, 1:-1, 1:-1]))
    cavity_rows = []
    if cavity.any():
        # padding keeps the order of the linear indices, so the smallest padded index of a cavity is its smallest point
        num, distinct = number(void_lab[1:-1, 1:-1, 1:-1][cavity])
        labels[cavity] = (CAVITY_BIT | num).astype(np.uint32)
        order = np.argsort(num, kind="stable")
        bounds = np.searchsorted(num[order], np.arange(len(distinct) + 1))
        pi, pj, pk = ii[cavity][order], jj[cavity][order], kk[cavity][order]
        cavity_rows = [mass_ref.moments_of_indices(pi[a:b], pj[a:b], pk[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    # the cubical complex
    a = inside
    V = int(np.count_nonzero(a))
    E = int(np.count_nonzero(a[:, :, :-1] & a[:, :, 1:]) + np.count_nonzero(a[:, :-1, :] & a[:, 1:, :]) + np.count_nonzero(a[:-1] & a[1:]))
    sq_xy = a[:, :-1, :-1] & a[:, :-1, 1:] & a[:, 1:, :-1] & a[:, 1:, 1:]
    sq_yz = a[:-1, :-1, :] & a[:-1, 1:, :] & a[1:, :-1, :] & a[1:, 1:, :]
    sq_xz = a[:-1, :, :-1] & a[:-1, :, 1:] & a[1:, :, :-1] & a[1:, :, 1:]
    F = int(np.count_nonzero(sq_xy) + np.count_nonzero(sq_yz) + np.count_nonzero(sq_xz))
    K = int(np.count_nonzero(sq_xy[:-1] & sq_xy[1:]))
    B, C = len(body_rows), len(cavity_rows)
    euler = V - E + F - K
    counts = dict(zip(COUNT_NAMES, (B, C, V, E, F, K, euler, B + C - euler, exterior_points)))
    return {"counts": counts, "body_rows": body_rows, "cavity_rows": cavity_rows, "labels": labels}


def solid(cc, words, origin, step, shape, level, max_dist=100.0):
    """topology() of the solid d < level on the lattice, d the oracle's map_scene (mass_ref.lattice_inside)."""
    return topology(mass_ref.lattice_inside(cc, words, origin, step, shape, level, max_dist))


def combine_rows(rows):
    """Rows combined entry by entry: sums for 0-9, minima for 10-12, maxima for 13-15 (the identity for no rows)."""
    out = [0] * 10 + [mass_ref.NO_MIN] * 3 + [0] * 3
    for r in rows:
        out = [out[e] + r[e] if e < 10 else min(out[e], r[e]) if e < 13 else max(out[e], r[e]) for e in range(16)]
    return out
