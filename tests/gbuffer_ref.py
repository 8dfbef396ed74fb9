"""The G-buffer contract of DESIGN.md section 14 in numpy: what rm_draw_gbuffer must write, to the last bit.

TEST INFRASTRUCTURE, written from the text of section 14 and not from the kernel.  It stands on the numpy oracle's map_scene
and fmax (oracle/rm_oracle_np.py) and restates everything else: rays, ray_march's loop, the taps, the shading normal and
diffuse term, the floor, and the per-pixel reduction.  Every numpy ufunc on float32 arrays is one binary32 operation per
element, sqrt and / are correctly rounded, nothing is fused.

The leaf of a surface sample is found without restating the operand rules: the program is re-tagged with one Material per
primitive (its ordinal, in two passes of 8 bits each), and map_scene's material -- which follows exactly the operand rules
of the ABI -- names the primitive.  Tags never change a distance.

per_sample(...) returns the records of one sample ray per pixel; reduce(...) applies section 14's rule to a list of them;
render(...) does both for rows of a frame and returns the twelve named arrays of RayMarchingResources.draw_gbuffer.

Nearest sample: the one that minimises (t, sample id) among samples with kind != RM_HIT_NONE.  t is never NaN in a march
that hits (a NaN distance can neither hit nor escape; the floor test t > 0 rejects NaN); +inf is possible for a floor ray and
compares as usual.  Should a NaN t ever appear, it counts as +inf here and in the kernel."""
import numpy as np

from oracle import rm_oracle_np as onp

F = np.float32
RM_NO_ID = 0xFFFFFFFF
RM_HIT_NONE, RM_HIT_SURFACE, RM_HIT_FLOOR = 0, 1, 2
RM_SAMPLE_CENTER, RM_SAMPLE_ALL = 16, 17
NPARAM = {0: 4, 1: 6, 2: 4, 10: 5, 100: 0, 101: 0, 102: 0, 110: 1, 200: 3, 201: 0, 202: 4, 203: 0, 204: 1, 205: 0, 300: 1}
PRIMS = (0, 1, 2, 10)
KEYS = ("t", "position", "normal", "diffuse", "kind", "sample", "leaf", "material", "surface_mask", "floor_mask",
        "selected_mask", "steps")


def _matvec(m, x, y, z, w):
    return tuple(((m[0 + r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * w for r in range(4))


def _normalize3(x, y, z):
    l = np.sqrt((x * x + y * y) + z * z)
    return x / l, y / l, z / l


def leaf_programs(cmd_count, words):
    """The program with its own tags dropped and Material(tag) after every primitive, for tag = ordinal & 255 and
    tag = ordinal >> 8: ((cmd_count, words) low, (cmd_count, words) high, command index of each primitive by ordinal)."""
    w = [int(x) for x in np.asarray(words, dtype=np.uint32)]
    lo, hi, prim_index, q, n = [], [], [], 0, 0
    for i in range(cmd_count):
        op = w[q]
        size = 1 + NPARAM[op]
        if op != 300:
            lo += w[q:q + size]
            hi += w[q:q + size]
            n += 1
            if op in PRIMS:
                k = len(prim_index)
                assert k < 65536
                prim_index.append(i)
                lo += [300, k & 255]
                hi += [300, k >> 8]
        q += size
    n += len(prim_index)
    return (n, np.asarray(lo, dtype=np.uint32)), (n, np.asarray(hi, dtype=np.uint32)), np.asarray(prim_index, dtype=np.uint32)


def leaf_and_material(cmd_count, words, max_dist, x, y, z):
    """(leaf, material) of map_scene's value at each point: rm_query_points' ids."""
    words = np.asarray(words, dtype=np.uint32)
    if cmd_count == 0:
        return np.full(x.shape, RM_NO_ID, dtype=np.uint32), np.zeros(x.shape, dtype=np.uint32)
    _, mat = onp.map_scene(cmd_count, words, max_dist, x, y, z, want_material=True)
    (nl, wl), (nh, wh), prim_index = leaf_programs(cmd_count, words)
    _, low = onp.map_scene(nl, wl, max_dist, x, y, z, want_material=True)
    high = 0
    if len(prim_index) > 256:
        _, high = onp.map_scene(nh, wh, max_dist, x, y, z, want_material=True)
    return prim_index[np.asarray(low, dtype=np.int64) + 256 * np.asarray(high, dtype=np.int64)], np.asarray(mat, dtype=np.uint32)


def camera_rays(px, py, sample, uniforms, W, H):
    """rm_camera_rays: origin (3 scalars) and direction (3 arrays) of sample `sample` (0..15 or RM_SAMPLE_CENTER)."""
    ve = np.asarray(uniforms["viewport_extent"], dtype=F)
    inv_proj, inv_view = np.asarray(uniforms["inv_proj"], dtype=F), np.asarray(uniforms["inv_view"], dtype=F)
    n = px.shape[0]
    ro = _matvec(inv_view, F(0), F(0), F(0), F(1))
    sx = ((px.astype(F) + F(0.5)) / F(W)) * F(2) - F(1)
    sy = F(1) - ((py.astype(F) + F(0.5)) / F(H)) * F(2)
    ox = oy = F(0)                                  # the pixel centre
    if sample < 16:
        i, j = sample // 4, sample % 4
        ox = ((F(i) + F(0.5)) / F(4) - F(0.5)) / ve[0] * F(2)
        oy = ((F(j) + F(0.5)) / F(4) - F(0.5)) / ve[1] * F(2)
    pv = _matvec(inv_proj, sx + ox, sy + oy, np.full(n, F(-1)), np.full(n, F(1)))
    pw = _matvec(inv_view, *pv)
    d = [pw[k] - ro[k] for k in range(4)]
    ln = np.sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3])
    return ro, (d[0] / ln, d[1] / ln, d[2] / ln)


def cast(cmd_count, words, limits, ro, dx, dy, dz):
    """rm_cast_rays for rays of one origin: dict of kind, steps, leaf, material (n,) uint32 and hit (n, 8) float32."""
    min_dist, max_dist, max_iter = F(limits[0]), F(limits[1]), int(limits[2])
    words = np.asarray(words, dtype=np.uint32)
    n = dx.shape[0]
    kind = np.zeros(n, dtype=np.uint32)
    steps = np.full(n, max_iter, dtype=np.uint32)
    leaf = np.full(n, RM_NO_ID, dtype=np.uint32)
    mat = np.full(n, RM_NO_ID, dtype=np.uint32)
    hit = np.zeros((n, 8), dtype=F)
    hit[:, 0] = np.inf                              # the miss record: +inf and zeros
    dist = np.zeros(n, dtype=F)
    alive = np.arange(n)
    for it in range(max_iter):                      # ray_march's loop
        if alive.size == 0:
            break
        d = dist[alive]
        qx, qy, qz = ro[0] + dx[alive] * d, ro[1] + dy[alive] * d, ro[2] + dz[alive] * d
        s = onp.map_scene(cmd_count, words, max_dist, qx, qy, qz)
        h = s < min_dist
        esc = ~h & (s > max_dist)
        hi = alive[h]
        kind[hi], steps[hi] = RM_HIT_SURFACE, it + 1
        hit[hi, 0], hit[hi, 1], hit[hi, 2], hit[hi, 3] = d[h], qx[h], qy[h], qz[h]
        steps[alive[esc]] = it + 1
        go = ~(h | esc)
        dist[alive[go]] = d[go] + s[go]
        alive = alive[go]
    sf = np.nonzero(kind == RM_HIT_SURFACE)[0]
    if sf.size:                                     # taps, shading normal and max(0.02, n.l) with the reference's light
        x, y, z = hit[sf, 1], hit[sf, 2], hit[sf, 3]
        e = F(0.0001)
        f0 = onp.map_scene(cmd_count, words, max_dist, x + e, y + -e, z + -e)
        f1 = onp.map_scene(cmd_count, words, max_dist, x + -e, y + -e, z + e)
        f2 = onp.map_scene(cmd_count, words, max_dist, x + -e, y + e, z + -e)
        f3 = onp.map_scene(cmd_count, words, max_dist, x + e, y + e, z + e)
        nx, ny, nz = _normalize3(((f0 + -f1) + -f2) + f3, ((-f0 + -f1) + f2) + f3, ((-f0 + f1) + -f2) + f3)
        lx, ly, lz = _normalize3(x - F(2.0), y - F(-5.0), z - F(3.0))
        hit[sf, 4], hit[sf, 5], hit[sf, 6] = nx, ny, nz
        hit[sf, 7] = onp.fmax(F(0.02), (nx * lx + ny * ly) + nz * lz)
        leaf[sf], mat[sf] = leaf_and_material(cmd_count, words, max_dist, x, y, z)
    ms = np.nonzero(kind == RM_HIT_NONE)[0]
    if ms.size:                                     # the floor
        t = (F(-1.5) - ro[1]) / dy[ms]
        on = t > 0
        fl, t = ms[on], t[on]
        kind[fl] = RM_HIT_FLOOR
        hit[fl, 0], hit[fl, 1], hit[fl, 2], hit[fl, 3] = t, ro[0] + dx[fl] * t, F(-1.5), ro[2] + dz[fl] * t
        hit[fl, 4], hit[fl, 5], hit[fl, 6], hit[fl, 7] = F(0), F(1), F(0), F(0)
    return {"kind": kind, "steps": steps, "leaf": leaf, "material": mat, "hit": hit}


def per_sample(px, py, sample, uniforms, limits, cmd_count, words, W, H):
    """The record of sample `sample` of pixels (px[i], py[i]): what rm_cast_rays returns for rm_camera_rays' ray."""
    with np.errstate(all="ignore"):
        ro, (dx, dy, dz) = camera_rays(np.asarray(px, dtype=np.uint32), np.asarray(py, dtype=np.uint32), sample, uniforms, W, H)
        return cast(cmd_count, words, limits, ro, dx, dy, dz)


def sample_ids(sample):
    if sample == RM_SAMPLE_ALL:
        return list(range(16))
    assert 0 <= sample <= RM_SAMPLE_CENTER
    return [sample]


def reduce(records, ids, select=None):
    """Section 14's reduction of the per-sample records `records` (dicts of per_sample, or of the same keys from
    rm_cast_rays; any iterable, consumed one record at a time) with sample ids `ids` (ascending) -> the twelve named arrays,
    each (n, ...)."""
    first, count = (0, 0) if select is None else select
    surface = floor = selected = steps = best_t = geom = out_ids = None
    last = -1
    for r, s in zip(records, ids):
        assert s > last                             # ascending ids: a tie on t keeps the lower id
        last = s
        kind, leaf = r["kind"], r["leaf"].astype(np.int64)
        if surface is None:
            n = kind.shape[0]
            surface, floor, selected, steps = (np.zeros(n, dtype=np.uint32) for _ in range(4))
            best_t = np.full(n, np.inf, dtype=F)
            geom = np.zeros((n, 8), dtype=F)
            geom[:, 0] = np.inf                     # no hit sample: the miss record
            out_ids = np.zeros((n, 4), dtype=np.uint32)
            out_ids[:, 1:] = RM_NO_ID               # ... and (RM_HIT_NONE, RM_NO_ID, RM_NO_ID, RM_NO_ID)
        bit = np.uint32(1 << s)
        is_s = kind == RM_HIT_SURFACE
        surface |= np.where(is_s, bit, np.uint32(0))
        floor |= np.where(kind == RM_HIT_FLOOR, bit, np.uint32(0))
        selected |= np.where(is_s & (leaf >= first) & (leaf < first + count), bit, np.uint32(0))
        steps += r["steps"]
        t = r["hit"][:, 0]
        t = np.where(np.isnan(t), F(np.inf), t)     # (no case known; section 14)
        take = (kind != RM_HIT_NONE) & ((out_ids[:, 0] == RM_HIT_NONE) | (t < best_t))
        best_t = np.where(take, t, best_t)
        geom[take] = r["hit"][take]
        out_ids[take, 0], out_ids[take, 1], out_ids[take, 2], out_ids[take, 3] = kind[take], s, r["leaf"][take], r["material"][take]
    return {"t": geom[:, 0], "position": geom[:, 1:4], "normal": geom[:, 4:7], "diffuse": geom[:, 7],
            "kind": out_ids[:, 0], "sample": out_ids[:, 1], "leaf": out_ids[:, 2], "material": out_ids[:, 3],
            "surface_mask": surface, "floor_mask": floor, "selected_mask": selected, "steps": steps}


def render(uniforms, limits, cmd_count, words, W, H, row0=0, rows=None, sample=RM_SAMPLE_ALL, select=None, detail=False):
    """Rows [row0, row0 + rows) of the G-buffer -> dict of the twelve named arrays, each (rows, W[, 3]); detail=True also
    returns the per-sample records."""
    rows = H - row0 if rows is None else rows
    py, px = np.meshgrid(np.arange(row0, row0 + rows, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    ids = sample_ids(sample)
    records = [per_sample(px.ravel(), py.ravel(), s, uniforms, limits, cmd_count, words, W, H) for s in ids]
    out = {k: v.reshape((rows, W) + v.shape[1:]) for k, v in reduce(records, ids, select).items()}
    return (out, records) if detail else out
