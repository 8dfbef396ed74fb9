#!/usr/bin/env python3
"""The direction weights of rm_surface_measures' AREA: for each of the 13 lattice directions the fraction
of the sphere that is nearer to +nu or -nu than to any other of the 26 directions (the spherical Voronoi cells of the 26
neighbours).

Closed form.  The octahedral group maps the 26 directions onto themselves; its fundamental domain is the spherical triangle T
with the corners a = (1,0,0), b = (1,1,0)/sqrt 2, c = (1,1,1)/sqrt 3 -- 1/48 of the sphere, one corner per kind of direction.
A point of T has its nearest direction among a, b and c, so the three cells cut T along the great circles u.(a-b) = 0,
u.(a-c) = 0, u.(b-c) = 0: three convex spherical polygons, each with the area (sum of its angles) - (n - 2) pi (Girard).  An
axis cell collects the piece at a from the 8 copies of T around it, and so on:
    w_axis = 2 * 8 * A_a / 4 pi,  w_face = 2 * 4 * A_b / 4 pi,  w_space = 2 * 6 * A_c / 4 pi,  3 w_axis + 6 w_face + 4 w_space = 1.
Everything is binary64 arithmetic on a handful of vectors: good to about 1e-15.

    python tools/surface_weights.py            prints the three constants as they stand in csrc/rm_abi.hip and tests/surface_ref.py
    python tools/surface_weights.py --check N  also integrates the cells on an N x 2N latitude-longitude grid (midpoint rule)"""
import argparse
import math

import numpy as np


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / math.sqrt(float(v @ v))


def clip(poly, normal):
    """The part of the convex spherical polygon `poly` (unit vectors in order) with u . normal >= 0."""
    out = []
    for i, p in enumerate(poly):
        q = poly[(i + 1) % len(poly)]
        dp, dq = float(p @ normal), float(q @ normal)
        if dp >= 0.0:
            out.append(p)
        if (dp > 0.0 > dq) or (dp < 0.0 < dq):
            x = np.cross(np.cross(p, q), normal)      # the edge's great circle meets the cutting one at +-x
            x = unit(x)
            mid = unit(p + q)
            out.append(x if float(x @ mid) > 0.0 else -x)
    return out


def area(poly):
    """Girard: the sum of the interior angles minus (n - 2) pi."""
    n, total = len(poly), 0.0
    for i in range(n):
        p, prev, nxt = poly[i], poly[i - 1], poly[(i + 1) % n]
        t1 = unit(prev - p * float(prev @ p))         # tangents at p towards its neighbours
        t2 = unit(nxt - p * float(nxt @ p))
        total += math.acos(max(-1.0, min(1.0, float(t1 @ t2))))
    return total - (n - 2) * math.pi


def weights():
    a, b, c = unit([1, 0, 0]), unit([1, 1, 0]), unit([1, 1, 1])
    tri = [a, b, c]
    cell_a = clip(clip(tri, a - b), a - c)
    cell_b = clip(clip(tri, b - a), b - c)
    cell_c = clip(clip(tri, c - a), c - b)
    A = [area(cell_a), area(cell_b), area(cell_c)]
    assert abs(sum(A) - 4.0 * math.pi / 48.0) < 1e-14, (A, 4.0 * math.pi / 48.0)
    return (16.0 * A[0] / (4.0 * math.pi), 8.0 * A[1] / (4.0 * math.pi), 12.0 * A[2] / (4.0 * math.pi))


def directions26():
    d = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)]
    v = np.array(d, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=1))[:, None], np.array([abs(i) + abs(j) + abs(k) for i, j, k in d])


def quadrature(n):
    """The three weights by the midpoint rule on n latitudes x 2n longitudes."""
    dirs, kind = directions26()
    th = (np.arange(n) + 0.5) * (math.pi / n)
    ph = (np.arange(2 * n) + 0.5) * (math.pi / n)
    w = np.zeros(4)
    for t in th:
        u = np.stack([math.sin(t) * np.cos(ph), math.sin(t) * np.sin(ph), np.full_like(ph, math.cos(t))], axis=1)
        near = kind[np.argmax(u @ dirs.T, axis=1)]
        w += np.bincount(near, minlength=4) * (math.sin(t) * (math.pi / n) ** 2)
    w /= 4.0 * math.pi
    return w[1] / 3.0, w[2] / 6.0, w[3] / 4.0        # per unsigned direction: 3 axes, 6 face and 4 space diagonals


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", type=int, default=0, metavar="N", help="also integrate on an N x 2N latitude-longitude grid")
    args = ap.parse_args()
    w = weights()
    for name, x in zip(("axis", "face diagonal", "space diagonal"), w):
        print("%-15s %.17g" % (name, x))
    print("3 w1 + 6 w2 + 4 w3 - 1 = %.3g" % (3.0 * w[0] + 6.0 * w[1] + 4.0 * w[2] - 1.0))
    if args.check:
        q = quadrature(args.check)
        print("quadrature %d x %d: %s; differences %s" % (args.check, 2 * args.check, " ".join("%.9f" % x for x in q),
                                                          " ".join("%.2e" % (x - y) for x, y in zip(q, w))))


if __name__ == "__main__":
    main()
