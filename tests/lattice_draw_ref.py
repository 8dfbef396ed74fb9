"""The lattice-draw contract of DESIGN.md section 28 in numpy: what rm_cast_lattice and rm_draw_lattice must write, to the last
bit.  Vectorised over rays, looping over events; every step is one rounded binary32 operation in the contract's order.

The traversal is written twice: walk() is the incremental walk (the cell, the three next planes, the smallest (t, axis) wins);
merge() is the definition -- per axis the monotone sequence of its plane crossings, the three sequences merged by (t, axis),
the cells along the merged order.  Neither knows about bricks: both visit every cell.  exact_cell() is the same geometry in
Fractions, for rays whose events are well separated.  cast() and draw() put the hit record, the miss (the floor of
rm_cast_rays) and fs_main's resolve around a traversal."""
from fractions import Fraction

import numpy as np

import gbuffer_ref
from oracle import rm_oracle_np as onp

F = np.float32
RM_NO_ID = 0xFFFFFFFF
RM_HIT_NONE, RM_HIT_SURFACE, RM_HIT_FLOOR = 0, 1, 2
FACE_NONE = 6
NONE = 3  # the axis of a record whose origin is inside its cell


def window_of(shape, window=None):
    """(lo, hi) int64[3] of a window (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z); None: the whole lattice.  shape is (nx, ny, nz)."""
    if window is None:
        return np.zeros(3, dtype=np.int64), np.asarray(shape, dtype=np.int64)
    w = np.asarray(window, dtype=np.int64).reshape(6)
    assert np.all(w[:3] < w[3:]) and np.all(w[3:] <= np.asarray(shape))
    return w[:3].copy(), w[3:].copy()


def plane_t(e, r, m):
    """t_a(m) = (((float)m - 0.5f) - e_a) * r_a, for arrays that broadcast."""
    with np.errstate(all="ignore"):
        return ((np.asarray(m).astype(F) - F(0.5)) - e) * r


class Entry:
    """Ray to index space and the entry: per ray and axis e, g, r, parallel, up; per ray whether it meets the window, T0, its
    first cell and the axis of the first record (NONE: the origin is inside)."""

    def __init__(self, rays, origin, step, lo, hi):
        rays = np.asarray(rays, dtype=F).reshape(-1, 6)
        o, s = np.asarray(origin, dtype=F), np.asarray(step, dtype=F)
        n = len(rays)
        with np.errstate(all="ignore"):
            self.e = (rays[:, 0:3] - o) / s
            self.g = rays[:, 3:6] / s
            self.r = F(1) / self.g
        self.par = (self.g == 0) | np.isinf(self.r)
        self.up = self.r > 0
        self.lo, self.hi = lo, hi
        meets = np.all(np.isfinite(self.e) & np.isfinite(self.g), axis=1)
        cell = np.zeros((n, 3), dtype=np.int64)
        T0, T1 = np.zeros(n, dtype=F), np.full(n, np.inf, dtype=F)
        tin = np.zeros((n, 3), dtype=F)
        for a in range(3):
            e, r, par, up = self.e[:, a], self.r[:, a], self.par[:, a], self.up[:, a]
            # a parallel axis: inside iff some m in [lo, hi) has m - 1/2 <= e < m + 1/2 (exact comparisons)
            m = np.arange(lo[a], hi[a])
            with np.errstate(invalid="ignore"):
                inside = (m[None, :].astype(F) - F(0.5) <= e[:, None]) & (e[:, None] < m[None, :].astype(F) + F(0.5))
            meets &= ~par | inside.any(axis=1)
            cell[:, a] = np.where(par, lo[a] + np.argmax(inside, axis=1), cell[:, a])
            tin[:, a] = plane_t(e, r, np.where(up, lo[a], hi[a]))
            tout = plane_t(e, r, np.where(up, hi[a], lo[a]))
            T0 = np.where(par, T0, onp.fmax(T0, tin[:, a]))
            T1 = np.where(par, T1, onp.fmin(T1, tout))
        with np.errstate(invalid="ignore"):
            meets &= T0 < T1
        axis = np.full(n, NONE, dtype=np.int64)
        for a in range(3):
            e, r, par, up = self.e[:, a], self.r[:, a], self.par[:, a], self.up[:, a]
            m = np.arange(lo[a] + 1, hi[a])                      # the planes strictly inside the window
            with np.errstate(invalid="ignore"):
                c = (plane_t(e[:, None], r[:, None], m[None, :]) <= T0[:, None]).sum(axis=1)
            cell[:, a] = np.where(par, cell[:, a], np.where(up, lo[a] + c, hi[a] - 1 - c))
            with np.errstate(invalid="ignore"):
                axis = np.where(~par & (tin[:, a] == T0), a, axis)
        self.meets, self.T0, self.cell, self.axis = meets, T0, cell, axis


def _occupied(classes, lo, hi, cell):
    """The class byte of each cell (n, 3) of (x, y, z) indices; points outside the window are empty."""
    inside = np.all((cell >= lo) & (cell < hi), axis=1)
    c = np.clip(cell, 0, np.asarray(classes.shape[::-1]) - 1)
    return np.where(inside, classes[c[:, 2], c[:, 1], c[:, 0]], 0)


def walk(classes, origin, step, rays, window=None):
    """The incremental walk.  classes: uint8 (nz, ny, nx).  Returns hit (n,) bool, t (n,) float32, axis (n,) (0..2, NONE), up
    (n,) bool (of the record's axis), cell (n, 3): the record of the hit cell; t, axis, up and cell mean nothing for a miss."""
    classes = np.asarray(classes)
    lo, hi = window_of(classes.shape[::-1], window)
    E = Entry(rays, origin, step, lo, hi)
    n = len(E.T0)
    cell, t, axis = E.cell.copy(), E.T0.copy(), E.axis.copy()
    hit = np.zeros(n, dtype=bool)
    alive = np.nonzero(E.meets)[0]
    for _ in range(int((hi - lo).sum()) + 1):                    # a ray takes at most nx + ny + nz events
        if alive.size == 0:
            break
        full = _occupied(classes, lo, hi, cell[alive]) != 0
        hit[alive[full]] = True
        alive = alive[~full]
        # each non-parallel axis offers its next plane; the smallest (t, a) wins, x < y < z on ties
        best = np.zeros(alive.size, dtype=F)
        best_a = np.full(alive.size, NONE, dtype=np.int64)
        plane = np.zeros(alive.size, dtype=np.int64)
        for a in range(3):
            up, par = E.up[alive, a], E.par[alive, a]
            p = np.where(up, cell[alive, a] + 1, cell[alive, a])
            ta = plane_t(E.e[alive, a], E.r[alive, a], p)
            with np.errstate(invalid="ignore"):
                take = ~par & ((best_a == NONE) | (ta < best))
            best, best_a, plane = np.where(take, ta, best), np.where(take, a, best_a), np.where(take, p, plane)
        rows = np.arange(alive.size)
        a_ = np.minimum(best_a, 2)
        up_ = E.up[alive, a_]
        leaving = plane == np.where(up_, hi[a_], lo[a_])
        go = (best_a != NONE) & ~leaving                         # no axis steps: the walk is its first cell
        cell[alive[go], a_[go]] += np.where(up_[go], 1, -1)
        t[alive[go]], axis[alive[go]] = best[go], best_a[go]
        alive = alive[go]
        del rows
    assert alive.size == 0
    up = E.up[np.arange(n), np.minimum(axis, 2)]
    return hit, t, axis, up, cell


def merge(classes, origin, step, rays, window=None):
    """The definition: the three monotone event sequences of a ray merged by (t, axis), a stable sort; the cells along them."""
    classes = np.asarray(classes)
    lo, hi = window_of(classes.shape[::-1], window)
    E = Entry(rays, origin, step, lo, hi)
    n = len(E.T0)
    hit, t, axis, cell = np.zeros(n, dtype=bool), E.T0.copy(), E.axis.copy(), E.cell.copy()
    for i in np.nonzero(E.meets)[0]:
        ts, axs, order, last = [], [], [], []
        for a in range(3):
            if E.par[i, a]:
                continue
            # the planes ahead of the first cell in the order of travel, the window's leaving plane the last
            planes = np.arange(E.cell[i, a] + 1, hi[a] + 1) if E.up[i, a] else np.arange(E.cell[i, a], lo[a] - 1, -1)
            ts.append(plane_t(E.e[i, a], E.r[i, a], planes))
            axs.append(np.full(len(planes), a))
            order.append(np.arange(len(planes)))
            last.append(np.arange(len(planes)) == len(planes) - 1)
        cells = E.cell[i][None, :]
        if ts:
            ts, axs, order, last = (np.concatenate(v) for v in (ts, axs, order, last))
            by = np.lexsort((order, axs, ts))
            ts, axs, last = ts[by], axs[by], last[by]
            k = int(np.argmax(last))                             # the first leaving plane ends the walk
            delta = np.zeros((k, 3), dtype=np.int64)
            delta[np.arange(k), axs[:k]] = np.where(E.up[i, axs[:k]], 1, -1)
            cells = np.concatenate([cells, E.cell[i][None, :] + np.cumsum(delta, axis=0)])
        full = _occupied(classes, lo, hi, cells) != 0
        if full.any():
            j = int(np.argmax(full))
            hit[i], cell[i] = True, cells[j]
            if j > 0:
                t[i], axis[i] = ts[j - 1], axs[j - 1]
    up = E.up[np.arange(n), np.minimum(axis, 2)]
    return hit, t, axis, up, cell


def exact_cell(classes, origin, step, ray, window=None, gap=Fraction(1, 1024)):
    """The hit cell of one ray in exact arithmetic on the binary32 inputs: (generic, hit, cell).  generic: no two events of the
    walk -- the entry and 0 among them -- closer than `gap` in t, and no direction component 0."""
    classes = np.asarray(classes)
    lo, hi = window_of(classes.shape[::-1], window)
    fr = lambda x: Fraction(float(x))  # noqa: E731
    O, D = [fr(x) for x in ray[:3]], [fr(x) for x in ray[3:]]
    o, s = [fr(x) for x in np.asarray(origin, dtype=F)], [fr(x) for x in np.asarray(step, dtype=F)]
    if any(d == 0 for d in D):
        return False, False, None
    e = [(O[a] - o[a]) / s[a] for a in range(3)]
    g = [D[a] / s[a] for a in range(3)]
    tp = lambda a, m: (Fraction(m) - Fraction(1, 2) - e[a]) / g[a]  # noqa: E731
    up = [g[a] > 0 for a in range(3)]
    tin = [tp(a, int(lo[a] if up[a] else hi[a])) for a in range(3)]
    tout = [tp(a, int(hi[a] if up[a] else lo[a])) for a in range(3)]
    T0, T1 = max([Fraction(0)] + tin), min(tout)
    events = sorted([Fraction(0)] + tin)
    generic = all(b - a >= gap for a, b in zip(events, events[1:])) and abs(T1 - T0) >= gap
    if T0 >= T1:
        return generic, False, None
    cell = []
    for a in range(3):
        x = e[a] + g[a] * T0 + Fraction(1, 2)                    # the point at T0, in cells
        planes = [tp(a, m) for m in range(int(lo[a]) + 1, int(hi[a]))]
        generic = generic and all(abs(p - T0) >= gap for p in planes)
        cell.append(min(max(int(x // 1), int(lo[a])), int(hi[a]) - 1))
    while True:
        if classes[cell[2], cell[1], cell[0]] != 0:
            return generic, True, tuple(cell)
        nxt = sorted((tp(a, cell[a] + 1 if up[a] else cell[a]), a) for a in range(3))
        generic = generic and nxt[1][0] - nxt[0][0] >= gap
        a = nxt[0][1]
        cell[a] += 1 if up[a] else -1
        if not lo[a] <= cell[a] < hi[a]:
            return generic, False, None


def palette_index(cls, count):
    """min(c, count - 1): the material of a class byte."""
    return np.minimum(np.asarray(cls, dtype=np.int64), count - 1)


def cast(classes, origin, step, rays, materials, window=None, traverse=walk):
    """rm_cast_lattice: dict of hit (n, 8) float32, ids (n, 4) uint32, rgb (n, 3) float32."""
    classes = np.asarray(classes)
    rays = np.asarray(rays, dtype=F).reshape(-1, 6)
    table = np.asarray(materials, dtype=F).reshape(-1, 3)
    n = len(rays)
    nx, ny = classes.shape[2], classes.shape[1]
    hit, t, axis, up, cell = traverse(classes, origin, step, rays, window)
    rec = np.zeros((n, 8), dtype=F)
    rec[:, 0] = np.inf
    ids = np.full((n, 4), RM_NO_ID, dtype=np.uint32)
    ids[:, 0] = RM_HIT_NONE
    rgb = np.zeros((n, 3), dtype=F)
    O, D = rays[:, 0:3], rays[:, 3:6]
    h = np.nonzero(hit)[0]
    if h.size:
        with np.errstate(all="ignore"):
            P = O[h] + D[h] * t[h][:, None]
            faced = axis[h] != NONE
            nrm = np.zeros((h.size, 3), dtype=F)
            nrm[np.nonzero(faced)[0], axis[h][faced]] = np.where(up[h][faced], F(-1), F(1))
            l = onp._normalize3(P[:, 0] - F(2.0), P[:, 1] - F(-5.0), P[:, 2] - F(3.0))          # shade_hit: n is a unit vector
            nn = onp._normalize3(nrm[:, 0], nrm[:, 1], nrm[:, 2])
            k = np.where(faced, onp.fmax(F(0.02), (nn[0] * l[0] + nn[1] * l[1]) + nn[2] * l[2]), F(0.02)).astype(F)
        cls = classes[cell[h, 2], cell[h, 1], cell[h, 0]].astype(np.uint32)
        rec[h, 0], rec[h, 1:4], rec[h, 4:7], rec[h, 7] = t[h], P, nrm, k
        ids[h, 0] = RM_HIT_SURFACE
        ids[h, 1] = (cell[h, 0] + nx * (cell[h, 1] + ny * cell[h, 2])).astype(np.uint32)
        ids[h, 2] = cls
        ids[h, 3] = np.where(faced, 2 * axis[h] + np.where(up[h], 0, 1), FACE_NONE).astype(np.uint32)
        rgb[h] = table[palette_index(cls, len(table))] * k[:, None]
    m = np.nonzero(~hit)[0]
    if m.size:                                                   # rm_cast_rays' miss (wgsl:117-130)
        with np.errstate(all="ignore"):
            fd = (F(-1.5) - O[m, 1]) / D[m, 1]
            on = fd > 0
            f, tf = m[on], fd[on]
            fx = O[f, 0] + D[f, 0] * tf
            fz = O[f, 2] + D[f, 2] * tf
            bit = ((onp.f2i(np.rint(fx + F(0.5))) ^ onp.f2i(np.rint(fz + F(0.5)))) & 1).astype(F)
        gg = F(0.2) * bit
        rgb[f, 0], rgb[f, 1], rgb[f, 2] = F(0.1) + gg, F(0.1) + gg, F(0.2) + gg
        rec[f, 0], rec[f, 1], rec[f, 2], rec[f, 3] = tf, fx, F(-1.5), fz
        rec[f, 4:7] = np.asarray([0.0, 1.0, 0.0], dtype=F)
        ids[f, 0] = RM_HIT_FLOOR
    return {"hit": rec, "ids": ids, "rgb": rgb}


def resolve(sample_rgb):
    """fs_main's accumulation: sample_rgb is a list of sixteen (n, 3) arrays in sample order -> (n, 4) float32."""
    total = np.zeros_like(sample_rgb[0])
    for c in sample_rgb:
        total = total + np.sqrt(c)
    out = np.ones((len(total), 4), dtype=F)
    out[:, :3] = total / F(16)
    return out


def unorm8(image, bgra=False):
    """An RGBA32F image in an 8-bit format: clamp (NaN -> 0), * 255, round to nearest even."""
    x = np.nan_to_num(np.asarray(image, dtype=F), nan=0.0)
    q = np.rint(np.clip(x, F(0), F(1)) * F(255)).astype(np.uint8)
    return q[..., [2, 1, 0, 3]] if bgra else q


def draw(classes, origin, step, materials, uniforms, W, H, row0=0, rows=None, window=None):
    """rm_draw_lattice in RGBA32F: (rows, W, 4) float32."""
    rows = H - row0 if rows is None else rows
    py, px = np.meshgrid(np.arange(row0, row0 + rows, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    px, py = px.ravel(), py.ravel()
    samples = []
    for s in range(16):
        ro, d = gbuffer_ref.camera_rays(px, py, s, uniforms, W, H)
        rays = np.stack([np.full(px.size, ro[0], dtype=F), np.full(px.size, ro[1], dtype=F), np.full(px.size, ro[2], dtype=F),
                         d[0], d[1], d[2]], axis=1).astype(F)
        samples.append(cast(classes, origin, step, rays, materials, window)["rgb"])
    return resolve(samples).reshape(rows, W, 4)
