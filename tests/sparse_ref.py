"""A numpy restatement of which bricks sparse mesh extraction keeps ("The skipping rule"), for the tests:
rm_sparse_probe_kernel's decision per brick, the evaluation count rm_extract_mesh_sparse reports, and the P at which it asks
rm_program_bound for L and E.  Positions in binary32 one rounded operation at a time (numpy never fuses), the probe value from
the numpy oracle (the kernels' distances are its bit patterns), the radius and the two comparisons in binary64 in the kernel's
order.  Test infrastructure only."""
import numpy as np

from oracle import rm_oracle_np as onp

F = np.float32
BRICK, TILE = 8, 9


def axis_coords(o, s, n):
    """o + (float)i * s: one rounded product, one rounded sum."""
    return F(o) + np.arange(n, dtype=np.float64).astype(F) * F(s)


def lattice_P(origin, step, shape):
    """The largest |coordinate| of the lattice as rm_extract_mesh_sparse forms it: the first and the last point per axis."""
    P = 0.0
    for a in range(3):
        last = F(origin[a]) + F(shape[a] - 1) * F(step[a])
        P = max(P, abs(float(F(origin[a]))), abs(float(last)))
    return P


def _axis_tiles(o, s, n):
    """Per brick along one axis: the tile's extent in points, its first and last coordinate, the probe coordinate (binary32)
    and the half-width about the probe (binary64)."""
    c = axis_coords(o, s, n)
    i0 = np.arange(0, n, BRICK)
    ext = np.minimum(TILE, n - i0)
    x0, x1 = c[i0], c[i0 + ext - 1]
    mid = x0 + (x1 - x0) * F(0.5)
    x0d, x1d, md = x0.astype(np.float64), x1.astype(np.float64), mid.astype(np.float64)
    return ext.astype(np.int64), mid, np.maximum(x1d - md, md - x0d)


def brick_model(cc, words, origin, step, shape, level, L, E, max_dist=100.0):
    """keep: (bz, by, bx) bool, True where the probe kernel keeps the brick; evaluations: the EVALUATIONS statistic (one probe per
    brick and every tile point of a kept brick)."""
    ex, cx, hx = _axis_tiles(origin[0], step[0], shape[0])
    ey, cy, hy = _axis_tiles(origin[1], step[1], shape[1])
    ez, cz, hz = _axis_tiles(origin[2], step[2], shape[2])
    pz, py, px = np.meshgrid(cz, cy, cx, indexing="ij")
    with np.errstate(all="ignore"):
        v = np.asarray(onp.map_scene(cc, words, F(max_dist), px.ravel(), py.ravel(), pz.ravel()), dtype=F).reshape(px.shape)
        HZ, HY, HX = np.meshgrid(hz, hy, hx, indexing="ij")
        r = np.sqrt(HX * HX + HY * HY + HZ * HZ)
        reach = np.float64(L) * r
        err2 = np.float64(2.0 * E)
        margin = (reach + err2) * (1.0 + 1.0e-9)
        clear = (np.abs(v.astype(np.float64) - np.float64(F(level))) > margin) & (err2 <= 0.5 * reach)
    keep = ~clear
    points = ez[:, None, None] * ey[None, :, None] * ex[None, None, :]
    return keep, int(keep.size + points[keep].sum())


def mixed_bricks(dist, level):
    """dist: (nz, ny, nx) lattice distances.  (bz, by, bx) bool: the brick's tile has points on both sides of `d < level`."""
    with np.errstate(invalid="ignore"):
        inside = np.ascontiguousarray(dist, dtype=F) < F(level)
    nz, ny, nx = inside.shape
    bz, by, bx = ((n + BRICK - 1) // BRICK for n in (nz, ny, nx))
    out = np.zeros((bz, by, bx), dtype=bool)
    for k in range(bz):
        for j in range(by):
            for i in range(bx):
                t = inside[k * BRICK:k * BRICK + TILE, j * BRICK:j * BRICK + TILE, i * BRICK:i * BRICK + TILE]
                out[k, j, i] = t.any() and not t.all()
    return out
