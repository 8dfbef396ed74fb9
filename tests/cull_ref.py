"""Binary64 geometry the culling bounds are measured against ("Direct tests of the culling bounds"): how
close a half-line o + t d^, t >= 0, comes to a leaf, whether it meets the margin zone the miss-test tables promise a cleared ray
stays out of, and an upper bound on the infimum of a whole program along it.  TEST INFRASTRUCTURE, written from the geometry: it
shares no code with the kernels (csrc/rm_kernel_v5.h), the decoder or the oracles; leaf and scene VALUES come from
tests/scene_f64.py.  Everything is vectorised over N half-lines; directions may have any non-zero length.

Why the searches are sound.  A leaf's value is phi(q(x)) with q convex in x (|x_i - c_i| - h_i, or the radial distance minus r)
and phi(q) = |max(q, 0)| + min(max_i q_i, 0), the signed distance to the negative orthant: convex and non-decreasing in every
q_i.  So the value is convex along a line, whatever the signs of the extents, and a bracketed search around the smallest of its
kinks finds the infimum.  Every number returned as an infimum is the value at a parameter that was actually evaluated, hence never
below the true infimum: `bound <= infimum` is a necessary condition for a lower bound, with no tolerance."""
import numpy as np

import scene_f64

SPHERE, BOX, PLANE, CYLINDER = 0, 1, 2, 10
_GOLD = 0.5 * (3.0 - np.sqrt(5.0))


def commands(cmd_count, words):
    """[(opcode, parameters as float64, open transform scopes)] of a program."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    out, at, depth = [], 0, 0
    for _ in range(cmd_count):
        op = int(w[at])
        n = scene_f64._PARAMS[op]
        raw = w[at + 1:at + 1 + n]
        at += 1 + n
        if op in (201, 203, 205):
            depth -= 1
        out.append((op, raw.view(np.float32).astype(np.float64), depth))
        if op in (200, 202, 204):
            depth += 1
    return out


def words_of(*cmds):
    """(cmd_count, words) of a program given as (opcode, [binary32 parameters]) pairs in wire order."""
    out = []
    for op, params in cmds:
        out += [op] + [int(x) for x in np.asarray(params, dtype=np.float32).view(np.uint32)]
    return len(cmds), np.asarray(out, dtype=np.uint32)


def unit(d):
    d = np.atleast_2d(np.asarray(d, dtype=np.float64))
    n = np.linalg.norm(d, axis=1, keepdims=True)
    assert np.all(n > 0.0) and np.all(np.isfinite(n)), "directions must be finite and non-zero"
    return d / n


def _rays(o, d):
    dh = unit(d)
    o = np.broadcast_to(np.asarray(o, dtype=np.float64), dh.shape)
    return o, dh


def leaf_along(op, a, o, dh, t):
    """Value of leaf (op, a) at o + t dh; t: (N,) or (N, K)."""
    t = np.asarray(t, dtype=np.float64)
    if t.ndim == 1:
        return scene_f64._leaf(op, a, o + t[:, None] * dh)
    n, k = t.shape
    p = o[:, None, :] + t[:, :, None] * dh[:, None, :]
    return scene_f64._leaf(op, a, p.reshape(-1, 3)).reshape(n, k)


def _kinks(op, a, o, dh):
    """(N, K) parameters at which the leaf's value along the half-line may have a kink, clipped to t >= 0, plus 0 and a far end
    beyond which the value only grows."""
    m = a[:3] - o
    ext = np.abs(a[3:6]) if op == BOX else np.array([abs(a[3]), abs(a[4]), abs(a[3])])
    far = np.linalg.norm(m, axis=1) + np.linalg.norm(ext) + 1.0
    cols = [np.zeros(len(o)), far, np.clip(np.einsum("ij,ij->i", m, dh), 0.0, far)]
    with np.errstate(divide="ignore", invalid="ignore"):
        axes = (0, 1, 2) if op == BOX else (1,)
        for i in axes:
            for s in (-1.0, 0.0, 1.0):           # the faces and the mid-plane (|x_i - c_i| has a kink there)
                cols.append((m[:, i] + s * ext[i]) / dh[:, i])
        if op == CYLINDER:                       # where the line crosses the radius in the x-z plane, and where it is closest to the axis
            dx, dz = dh[:, 0], dh[:, 2]
            A = dx * dx + dz * dz
            B = m[:, 0] * dx + m[:, 2] * dz
            C = m[:, 0] ** 2 + m[:, 2] ** 2 - a[3] * a[3]
            disc = np.sqrt(np.maximum(B * B - A * C, 0.0))
            cols += [B / A, (B - disc) / A, (B + disc) / A]
    k = np.stack(cols, axis=1)
    k = np.where(np.isfinite(k), k, 0.0)
    return np.sort(np.clip(k, 0.0, far[:, None]), axis=1)


def _golden(f, lo, hi, iters=90):
    """Golden-section search of a function that is convex on [lo, hi] (arrays).  Returns (t, f(t)) of the best point evaluated."""
    x1, x2 = lo + _GOLD * (hi - lo), hi - _GOLD * (hi - lo)
    f1, f2 = f(x1), f(x2)
    bt, bv = np.where(f1 <= f2, x1, x2), np.minimum(f1, f2)
    for _ in range(iters):
        left = f1 <= f2
        hi = np.where(left, x2, hi)
        lo = np.where(left, lo, x1)
        xn = np.where(left, lo + _GOLD * (hi - lo), hi - _GOLD * (hi - lo))      # the one new point of this step
        fn = f(xn)
        x1, x2, f1, f2 = np.where(left, xn, x2), np.where(left, x1, xn), np.where(left, fn, f2), np.where(left, f1, fn)
        better = fn < bv
        bt, bv = np.where(better, xn, bt), np.where(better, fn, bv)
    return bt, bv


def closest_approach(op, a, o, d):
    """(infimum over t >= 0 of the leaf's value along o + t d^, the parameter where it is attained), (N,) each.  A Plane the
    half-line descends towards has infimum -inf at t = +inf."""
    a = np.asarray(a, dtype=np.float64)
    o, dh = _rays(o, d)
    if op == SPHERE:
        t = np.maximum(np.einsum("ij,ij->i", a[:3] - o, dh), 0.0)
        return leaf_along(op, a, o, dh, t), t
    if op == PLANE:
        v0, slope = o @ a[:3] + a[3], dh @ a[:3]
        return np.where(slope >= 0.0, v0, -np.inf), np.where(slope >= 0.0, 0.0, np.inf)
    assert op in (BOX, CYLINDER)
    k = _kinks(op, a, o, dh)
    v = leaf_along(op, a, o, dh, k)
    i = np.argmin(v, axis=1)
    rows = np.arange(len(o))
    bt, bv = k[rows, i], v[rows, i]
    # the nearest DISTINCT kinks on either side (clipping to [0, far] makes duplicates)
    lo = np.where(k < bt[:, None], k, -np.inf).max(axis=1)
    hi = np.where(k > bt[:, None], k, np.inf).min(axis=1)
    lo, hi = np.where(np.isfinite(lo), lo, bt), np.where(np.isfinite(hi), hi, bt)
    # convex: the minimum lies in one of the two intervals next to the smallest kink; each is searched on its own (the value is
    # smooth inside an interval, the kink between them is evaluated above)
    for p, q in ((lo, bt.copy()), (bt.copy(), hi)):
        t, val = _golden(lambda x: leaf_along(op, a, o, dh, x), p, q)
        better = val < bv
        bt, bv = np.where(better, t, bt), np.where(better, val, bv)
    return bv, bt


# ---- the zone of the miss-test tables -------------------------------------------------------------------------------------------
def cull_margin(c, rho, ro, min_dist, slack):
    """cull_margin of csrc/rm_kernel_v5.h as a real number: (max(min_dist, 0) + slack) 1.01 + 1e-4 (1 + |c|_1 + rho + |ro|_1 + slack)."""
    scale = 1.0 + float(np.abs(np.asarray(c, dtype=np.float64)).sum()) + float(rho) + float(np.abs(np.asarray(ro, dtype=np.float64)).sum()) + float(slack)
    return (max(float(min_dist), 0.0) + float(slack)) * 1.01 + 1.0e-4 * scale


def ball_distance(c, o, d):
    """Distance from the point c to the half-line, (N,)."""
    o, dh = _rays(o, d)
    m = np.asarray(c, dtype=np.float64) - o
    t = np.maximum(np.einsum("ij,ij->i", m, dh), 0.0)
    return np.linalg.norm(m - t[:, None] * dh, axis=1)


def meets_ball(c, R, o, d):
    return ball_distance(c, o, d) <= R


def meets_box(c, h, o, d):
    """Does the half-line meet the closed box [c - h, c + h] (h >= 0)?  Exact slab intervals: a zero component keeps or empties
    its slab, nothing is divided by it."""
    o, dh = _rays(o, d)
    c, h = np.asarray(c, dtype=np.float64), np.asarray(h, dtype=np.float64)
    tn, tf = np.zeros(len(o)), np.full(len(o), np.inf)
    for i in range(3):
        lo, hi, di = (c[i] - h[i]) - o[:, i], (c[i] + h[i]) - o[:, i], dh[:, i]
        zero = di == 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = lo / di, hi / di
        a, b = np.minimum(t1, t2), np.maximum(t1, t2)
        inside = (lo <= 0.0) & (hi >= 0.0)
        a = np.where(zero, np.where(inside, -np.inf, np.inf), a)
        b = np.where(zero, np.where(inside, np.inf, -np.inf), b)
        tn, tf = np.maximum(tn, a), np.minimum(tf, b)
    return tn <= tf


def zone(op, a, ro, min_dist, slack, shrink=0.0):
    """The zone of one table entry as ("ball", centre, radius) or ("box", centre, half extents): sphere max(r, 0) + M; box
    h+ + M; cylinder its bounding box (r, hh, r)+ + M.  M is lowered by the relative amount `shrink`."""
    a = np.asarray(a, dtype=np.float64)
    if op == SPHERE:
        rho = max(a[3], 0.0)
        return "ball", a[:3], rho + cull_margin(a[:3], rho, ro, min_dist, slack) * (1.0 - shrink)
    h = np.maximum(a[3:6], 0.0) if op == BOX else np.maximum(np.array([a[3], a[4], a[3]]), 0.0)
    return "box", a[:3], h + cull_margin(a[:3], h.sum(), ro, min_dist, slack) * (1.0 - shrink)


def meets_zone(z, o, d):
    return meets_ball(z[1], z[2], o, d) if z[0] == "ball" else meets_box(z[1], z[2], o, d)


# ---- a whole program -------------------------------------------------------------------------------------------------------------
def scene_infimum(cmd_count, words, o, d, max_dist=100.0, grid=96, refine=3, iters=40):
    """An upper bound on inf over t >= 0 of map_scene(o + t d^), (N,), and the parameter it was found at.  The smallest of the
    program's values at t = 0, at every world-space leaf's closest-approach parameter, on a uniform grid that ends beyond the
    farthest bounded leaf, and at a golden-section refinement around the `refine` best of those."""
    o, dh = _rays(o, d)
    n = len(o)
    cand, far = [np.zeros(n)], np.full(n, 1.0)
    for op, a, depth in commands(cmd_count, words):
        if op not in (SPHERE, BOX, PLANE, CYLINDER):
            continue
        if op != PLANE and np.all(np.isfinite(a)):
            far = np.maximum(far, np.linalg.norm(a[:3] - o, axis=1) * (2.0 if depth else 1.0) + np.abs(a[3:]).sum() + 1.0)
        if depth == 0 and op != PLANE and np.all(np.isfinite(a)):
            cand.append(closest_approach(op, a, o, dh)[1])
    far = far * 1.5
    ts = np.concatenate([np.stack(cand, axis=1), np.linspace(0.0, 1.0, grid)[None, :] * far[:, None]], axis=1)

    def f(t):
        t = np.asarray(t)
        if t.ndim == 1:
            return scene_f64.map_scene(cmd_count, words, max_dist, o + t[:, None] * dh)
        p = o[:, None, :] + t[:, :, None] * dh[:, None, :]
        return scene_f64.map_scene(cmd_count, words, max_dist, p.reshape(-1, 3)).reshape(t.shape)

    v = f(ts)
    v = np.where(np.isnan(v), np.inf, v)
    rows = np.arange(n)
    i0 = np.argmin(v, axis=1)
    bt, bv = ts[rows, i0], v[rows, i0]
    step = far / (grid - 1)
    for i in np.argsort(v, axis=1)[:, :refine].T:
        c = ts[rows, i]
        t, val = _golden(f, np.maximum(c - step, 0.0), c + step, iters=iters)
        better = val < bv
        bt, bv = np.where(better, t, bt), np.where(better, val, bv)
    return bv, bt
