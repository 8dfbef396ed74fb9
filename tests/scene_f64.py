"""map_scene in binary64, for the tests: the value the binary32 paths (the kernels, oracle/rm_oracle.c, oracle/rm_oracle_np.py)
are measured against when the question is how far they stray from the real-arithmetic distance ("The
evaluation error").  Written from the node definitions (wgsl:187-203), not from the oracles: positions are
(N, 3) arrays, leaves are written with vector norms, and nothing is rounded to binary32 after the parameters are read.  The
parameter words are binary32 numbers and widen exactly; every operation after that is a binary64 one, so the result is within a
few 2^-53 relative roundings of the real value -- nine orders of magnitude below the binary32 errors it is used to measure.
Finite programs only: NaN and signed-zero conventions are not reproduced."""
import numpy as np

_PARAMS = {0: 4, 1: 6, 2: 4, 10: 5, 100: 0, 101: 0, 102: 0, 110: 1, 200: 3, 201: 0, 202: 4, 203: 0, 204: 1, 205: 0, 300: 1}


def _positive_part_norm(q):
    return np.linalg.norm(np.maximum(q, 0.0), axis=1)


def _leaf(op, a, p):
    if op == 0:        # Sphere: centre, radius
        return np.linalg.norm(p - a[:3], axis=1) - a[3]
    if op == 1:        # Box: centre, half extents
        q = np.abs(p - a[:3]) - a[3:6]
        return _positive_part_norm(q) + np.minimum(q.max(axis=1), 0.0)
    if op == 2:        # Plane: normal (as given), offset
        return p @ a[:3] + a[3]
    # Cylinder about y: centre, radius, half height
    q = np.stack([np.hypot(p[:, 0] - a[0], p[:, 2] - a[2]) - a[3], np.abs(p[:, 1] - a[1]) - a[4]], axis=1)
    return _positive_part_norm(q) + np.minimum(q.max(axis=1), 0.0)


def _combine(op, a, lhs, rhs):
    if op == 100:
        return np.minimum(lhs, rhs)
    if op == 101:
        return np.maximum(lhs, -rhs)
    if op == 102:
        return np.maximum(lhs, rhs)
    k = a[0]           # SmoothUnion; k <= 0: the plain minimum
    if not k > 0.0:
        return np.minimum(lhs, rhs)
    h = np.maximum(k - np.abs(lhs - rhs), 0.0) / k
    return np.minimum(lhs, rhs) - h * h * k / 4.0


def map_scene(cmd_count, words, max_dist, points):
    """points: (N, 3), any float type (widened exactly).  Returns (N,) float64."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    p = np.array(points, dtype=np.float64).reshape(-1, 3)
    if cmd_count == 0:
        return np.full(len(p), float(max_dist))
    values, scopes, at = [], [], 0
    for _ in range(cmd_count):
        op = int(w[at])
        a = w[at + 1:at + 1 + _PARAMS[op]].view(np.float32).astype(np.float64)
        at += 1 + _PARAMS[op]
        if op == 200:
            scopes.append((p, 1.0))
            p = p - a[:3]
        elif op == 202:
            scopes.append((p, 1.0))
            t = 2.0 * np.cross(p, a[1:4])
            p = p + a[0] * t + np.cross(t, a[1:4])
        elif op == 204:
            scopes.append((p, a[0]))
            p = p / a[0]
        elif op in (201, 203, 205):
            p, s = scopes.pop()
            if op == 205:
                values[-1] = values[-1] * s
        elif op == 300:
            pass       # a material tag does not change the distance
        elif op in (0, 1, 2, 10):
            values.append(_leaf(op, a, p))
        else:
            rhs = values.pop()
            values.append(_combine(op, a, values.pop(), rhs))
    return values.pop()
