"""The traversal contract of DESIGN.md section 18 in numpy: what rm_trace_rays must write, to the last bit.

TEST INFRASTRUCTURE, written from the text of section 18 and not from the kernel.  It stands on the numpy oracle's map_scene,
fmin and fmax (oracle/rm_oracle_np.py) and restates the loop; the attributes of an event are rm_query_points' at its position
(gbuffer_ref.leaf_and_material, the taps as light_ref restates them).  Every numpy ufunc on float32 arrays is one binary32
operation per element, / is correctly rounded, nothing is fused.

trace(...) returns the sixteen named arrays of RayMarchingResources.trace_rays, vectorised over rays as light_ref.shadow is:
every live ray takes one step per pass, so `steps` is the pass number for all of them."""
import numpy as np

import gbuffer_ref
from oracle import rm_oracle_np as onp

F = np.float32
RM_NO_ID = 0xFFFFFFFF
RM_TRACE_ENTER, RM_TRACE_EXIT = 1, 2
RM_TRACE_START_INSIDE, RM_TRACE_END_INSIDE, RM_TRACE_OUT_OF_STEPS = 1, 2, 4
NAMES = ("t_min", "t_max", "min_step", "step_scale", "level", "max_steps")          # enum rm_trace, in order
DEFAULTS = (0.0, 100.0, 0.001, 1.0, 0.0, 1024.0)
KEYS = ("events", "steps", "flags", "stored", "t_end", "length", "d_start", "d_end", "t", "position", "normal", "width", "kind",
        "step", "leaf", "material")


def params(**named):
    """The six parameters as float32: the defaults with the named ones replaced."""
    p = np.array(DEFAULTS, dtype=F)
    for k, v in named.items():
        p[NAMES.index(k)] = v
    return p


def _normalize3(x, y, z):
    l = np.sqrt((x * x + y * y) + z * z)
    return x / l, y / l, z / l


def normals_at(cc, words, max_dist, x, y, z):
    """rm_query_points' normal: the four taps, summed and normalised as the shading does."""
    e = F(0.0001)
    f0 = onp.map_scene(cc, words, max_dist, x + e, y + -e, z + -e)
    f1 = onp.map_scene(cc, words, max_dist, x + -e, y + -e, z + e)
    f2 = onp.map_scene(cc, words, max_dist, x + -e, y + e, z + -e)
    f3 = onp.map_scene(cc, words, max_dist, x + e, y + e, z + e)
    return _normalize3(((f0 + -f1) + -f2) + f3, ((-f0 + -f1) + f2) + f3, ((-f0 + f1) + -f2) + f3)


def trace(cc, words, max_dist, rays, p=None, max_events=8, normals=False, ids=False):
    """rm_trace_rays for (n, 6) rays -> dict of KEYS.  p: the six parameters (None: the defaults); max_dist: the limits'
    (what an empty program's map_scene returns)."""
    p = params() if p is None else np.asarray(p, dtype=F)
    assert p.shape == (6,)
    t_min, t_max, min_step, scale, level, max_steps = p[0], p[1], p[2], p[3], p[4], int(p[5])
    K = int(max_events)
    words = np.asarray(words, dtype=np.uint32)
    max_dist = F(max_dist)
    rays = np.asarray(rays, dtype=F).reshape(-1, 6)
    n = rays.shape[0]
    ox, oy, oz, dx, dy, dz = (rays[:, k].copy() for k in range(6))

    ev = np.zeros((n, K, 8), dtype=F)
    ev[:, :, 0] = np.inf                                    # an unfilled slot: (+inf, 0, ..., 0)
    ev_ids = np.zeros((n, K, 4), dtype=np.uint32)
    ev_ids[:, :, 2:] = RM_NO_ID                             # ... and (0, 0, RM_NO_ID, RM_NO_ID)
    with np.errstate(all="ignore"):
        def D(i, tt):
            return onp.map_scene(cc, words, max_dist, ox[i] + dx[i] * tt, oy[i] + dy[i] * tt, oz[i] + dz[i] * tt)

        everyone = np.arange(n)
        t = np.full(n, t_min, dtype=F)
        da = np.asarray(D(everyone, t), dtype=F)
        inside = da < level
        steps = np.ones(n, dtype=np.uint32)
        events = np.zeros(n, dtype=np.uint32)
        length = np.zeros(n, dtype=F)
        t_enter = t.copy()
        start_inside, d_start = inside.copy(), da.copy()
        alive = everyone[t < t_max]
        for step in range(2, max_steps + 1):                # while t < T_MAX and steps < MAX_STEPS
            if alive.size == 0:
                break
            ta, a = t[alive], da[alive]
            h = onp.fmax(np.abs(a - level) * scale, min_step)
            tn = onp.fmin(ta + h, t_max)
            b = np.asarray(D(alive, tn), dtype=F)
            steps[alive] = step
            inb = b < level
            x = inb != inside[alive]
            if x.any():
                i = alive[x]
                tc = onp.fmin(ta[x] + (tn[x] - ta[x]) * ((a[x] - level) / (a[x] - b[x])), tn[x])
                w = tn[x] - ta[x]
                st = events[i] < K
                j, slot = i[st], events[i][st]
                ev[j, slot, 0] = tc[st]
                ev[j, slot, 1] = ox[j] + dx[j] * tc[st]
                ev[j, slot, 2] = oy[j] + dy[j] * tc[st]
                ev[j, slot, 3] = oz[j] + dz[j] * tc[st]
                ev[j, slot, 7] = w[st]
                ev_ids[j, slot, 0] = np.where(inb[x][st], RM_TRACE_ENTER, RM_TRACE_EXIT)
                ev_ids[j, slot, 1] = step
                events[i] += 1
                enter = inb[x]
                t_enter[i[enter]] = tc[enter]
                out = i[~enter]
                length[out] = length[out] + (tc[~enter] - t_enter[out])
            t[alive], da[alive], inside[alive] = tn, b, inb
            alive = alive[tn < t_max]
        length[inside] = length[inside] + (t[inside] - t_enter[inside])
        stored = np.minimum(events, K).astype(np.uint32)
        flags = (np.where(start_inside, RM_TRACE_START_INSIDE, 0) | np.where(inside, RM_TRACE_END_INSIDE, 0)
                 | np.where(t < t_max, RM_TRACE_OUT_OF_STEPS, 0)).astype(np.uint32)
        filled = np.arange(K)[None, :] < stored[:, None]
        if filled.any() and (normals or ids):
            x, y, z = ev[:, :, 1][filled], ev[:, :, 2][filled], ev[:, :, 3][filled]
            if normals:
                nx, ny, nz = normals_at(cc, words, max_dist, x, y, z)
                ev[:, :, 4][filled], ev[:, :, 5][filled], ev[:, :, 6][filled] = nx, ny, nz
            if ids:
                leaf, mat = gbuffer_ref.leaf_and_material(cc, words, max_dist, x, y, z)
                ev_ids[:, :, 2][filled], ev_ids[:, :, 3][filled] = leaf, mat
    return {"events": events, "steps": steps, "flags": flags, "stored": stored, "t_end": t, "length": length, "d_start": d_start,
            "d_end": da, "t": ev[:, :, 0], "position": ev[:, :, 1:4], "normal": ev[:, :, 4:7], "width": ev[:, :, 7],
            "kind": ev_ids[:, :, 0], "step": ev_ids[:, :, 1], "leaf": ev_ids[:, :, 2], "material": ev_ids[:, :, 3]}


def standard_rays(n=2001, seed=2):
    """The standard ray set: origins uniform in [-1.2, 1.2]^3, directions normalised Gaussians."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.2, 1.2, (n, 3)).astype(F)
    d = rng.normal(0, 1, (n, 3)).astype(F)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    return np.ascontiguousarray(np.concatenate([o, d], axis=1))


STANDARD = dict(t_min=0.25, t_max=6.0, min_step=0.005, step_scale=1.0)
# the three configurations of the issue: (parameters beyond STANDARD, K)
CONFIGS = {"level0": (dict(level=0.0, max_steps=4096), 8),
           "many_events": (dict(level=-0.05, max_steps=4096), 2),
           "out_of_steps": (dict(level=0.1, max_steps=24), 8)}


def config(name):
    named, K = CONFIGS[name]
    return params(**dict(STANDARD, **named)), K
