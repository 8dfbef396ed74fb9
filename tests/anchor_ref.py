"""The anchored pruning threshold of a ray's first own step (rm_kernel_v5.h "Pruning", anchored first step):
a binary32 restatement of the two device functions, the programs and the pairs of points the tests hold it to
(tests/test_anchor_cpu.py against binary64 geometry, tests/test_gpu_anchor.py against rm_selftest_anchor).

    aT       = |F_a| * 1.00001f + 4e-6f * (prune_scale + |p_a|_1)                         anchor_reach
    thr_base = min(thr_base, fma(|q - p_a|_1, 1.00001f, aT))                              anchor_thr_base
    thr      = thr_base + 4e-6f * (prune_scale + |q|_1)                                   the step's own position term

prune_scale = scene_scale + |ro|_1.  Every operation is one binary32 operation in the device's order.  The multiply-add is
formed in binary64 (the product of two binary32 numbers is exact there) and rounded twice, so it may differ from the device's
single rounding by one unit in the last place, in either direction: the GPU test compares with that allowance, the soundness
claims are made on the device's own numbers."""
import numpy as np

import cull_ref as R
import scenes

F = np.float32
K_PRUNE_ABS = F(4.0e-6)
ONE_UP = F(1.00001)
INF = F(np.inf)
E_REL = 4.0e-7          # "Pruning": the evaluation error is at most 4e-7 of scene_scale + |ro|_1 + |q|_1


def l1(p):
    p = np.abs(np.asarray(p, dtype=F))
    return (p[..., 0] + p[..., 1]) + p[..., 2]


def prune_scale(scene_scale, ro):
    return F(F(scene_scale) + l1(ro))


def anchor_reach(a, sd, ps):
    with np.errstate(all="ignore"):
        return (np.abs(np.asarray(sd, dtype=F)) * ONE_UP + K_PRUNE_ABS * (F(ps) + l1(a))).astype(F)


def anchor_thr_base(thr_base, q, a, aT):
    q, a = np.asarray(q, dtype=F), np.asarray(a, dtype=F)
    with np.errstate(all="ignore"):
        d = np.abs(q - a)
        dist = (d[..., 0] + d[..., 1]) + d[..., 2]
        t = (dist.astype(np.float64) * np.float64(ONE_UP) + np.asarray(aT, dtype=F).astype(np.float64)).astype(F)
        old = np.broadcast_to(np.asarray(thr_base, dtype=F), t.shape)
        return np.where(t < old, t, old).astype(F)      # a NaN t leaves the old value


def step_threshold(thr_base, q, ps):
    with np.errstate(all="ignore"):
        return (np.asarray(thr_base, dtype=F) + K_PRUNE_ABS * (F(ps) + l1(q))).astype(F)


def threshold(q, a, sd, ps, thr_base=INF):
    """what the march hands to the culling at q, anchored at (a, sd)"""
    return step_threshold(anchor_thr_base(thr_base, q, a, anchor_reach(a, sd, ps)), q, ps)


def eval_error(ps, p):
    """the bound of "Pruning" on |F_computed - F| at p, in binary64"""
    return E_REL * (float(ps) + np.abs(np.asarray(p, dtype=np.float64)).sum(axis=-1))


# ---- programs ---------------------------------------------------------------------------------------------------------------------
FAR = (1000.0, -1000.0, 1000.0)


def _shifted(scene, off):
    nodes, root = scene
    out = []
    for kind, p, lhs, rhs in nodes:
        p = list(p)
        if kind in (scenes.SPHERE, scenes.BOX):
            p[:3] = [p[0] + off[0], p[1] + off[1], p[2] + off[2]]
        out.append((kind, p, lhs, rhs))
    return out, root


def tiny_sphere():
    """a sphere smaller than a 2x2 block of a 64x64 frame's pixels beside empty space, and a box off to one side"""
    t = scenes._Tab()
    return t.nodes, t.op(scenes.UNION, t.sphere((0.0, 0.0, 0.0), 0.04), t.box((1.6, 0.2, -0.3), (0.35, 0.5, 0.3)))


def edge_on_box():
    """a slab 8 mm thick whose plane passes (nearly) through the camera: drawn with EDGE_ON_EVENTS, the orbit camera at its starting
    position on the z axis, the slab at x = 0.26 is seen at 3 degrees -- a sliver three pixels wide down one column of tiles of a
    64x64 frame, three pixels from their border"""
    t = scenes._Tab()
    slab = t.box((0.26, 0.0, 0.0), (0.004, 1.2, 1.2))
    return t.nodes, t.op(scenes.UNION, t.op(scenes.SUBTRACTION, slab, t.sphere((0.26, 0.6, 0.0), 0.3)), t.sphere((-0.9, -1.0, 0.4), 0.2))


EDGE_ON_EVENTS = ()     # no orbit event: OrbitCameraController::new's camera


def far_scene():
    return _shifted(scenes.g32(), FAR)


def degenerate():
    """radii zero and negative, a flat and a line box"""
    t = scenes._Tab()
    prims = [t.sphere((0.0, 0.0, 0.0), 0.0), t.sphere((0.9, 0.1, 0.0), -0.25), t.box((-0.8, 0.0, 0.3), (0.5, 0.0, 0.5)),
             t.box((0.0, 0.7, -0.6), (0.0, 0.0, 0.4)), t.sphere((0.2, -0.6, 0.5), 0.3)]
    return t.nodes, scenes._fold_left(t, prims)


# name -> (scene, centre the cameras orbit)
PROGRAMS = {
    "g32": (scenes.g32, (0.0, 0.0, 0.0)),
    "g64": (scenes.g64, (0.0, 0.0, 0.0)),
    "g32_balanced": (scenes.g32_balanced, (0.0, 0.0, 0.0)),
    "far": (far_scene, FAR),
    "degenerate": (degenerate, (0.0, 0.0, 0.0)),
    "tiny_sphere": (tiny_sphere, (0.0, 0.0, 0.0)),
    "edge_on_box": (edge_on_box, (0.0, 0.0, 0.0)),
}
PAIR_PROGRAMS = ("g32", "g64", "g32_balanced", "far", "degenerate")


def program(oracle, name):
    """-> (cmd_count, words uint32, centre float64)"""
    scene, centre = PROGRAMS[name]
    cc, w = oracle.serialize(*scene())
    return cc, np.asarray(w, dtype=np.uint32), np.asarray(centre, dtype=np.float64)


# ---- pairs ------------------------------------------------------------------------------------------------------------------------
def pairs(ro, centre, f0, rng, n):
    """(n, 2, 3) binary32: [:, 0] the anchor a, [:, 1] the evaluation point q.  A third on a common start sphere |p - ro| = f0 a
    few pixels to a quarter of the frame apart (what the march meets); the rest anywhere: in and around the scene at
    separations 1e-6 .. 10, identical points, the anchor on a surface, the two on opposite sides of the scene."""
    ro, centre = np.asarray(ro, dtype=np.float64), np.asarray(centre, dtype=np.float64)
    k = n // 3
    fwd = R.unit(centre - ro)[0]
    d1 = R.unit(fwd[None] + rng.normal(size=(k, 3)) * 0.35)
    d2 = R.unit(d1 + rng.normal(size=(k, 3)) * 10.0 ** rng.uniform(-4.0, -0.5, size=(k, 1)))
    on = np.stack([ro + d1 * f0, ro + d2 * f0], axis=1)
    m = n - k
    a = centre + rng.uniform(-3.0, 3.0, size=(m, 3))
    q = a + R.unit(rng.normal(size=(m, 3))) * 10.0 ** rng.uniform(-6.0, 1.0, size=(m, 1))
    q[::7] = a[::7]                                        # the same point
    q[1::7] = 2.0 * centre - a[1::7]                       # across the scene
    a[2::7] = centre + (a[2::7] - centre) * 0.2            # inside the scene's body: values near zero and negative
    return np.concatenate([on, np.stack([a, q], axis=1)]).astype(F)


NON_FINITE = (np.nan, np.inf, -np.inf)


def poisoned(pr, rng):
    """pairs with one coordinate of a or of q replaced by a NaN or an infinity; in some, the same infinity in both points"""
    out = np.array(pr, dtype=F, copy=True)
    for i in range(len(out)):
        which, k, v = int(rng.integers(3)), int(rng.integers(3)), F(NON_FINITE[int(rng.integers(3))])
        if which < 2:
            out[i, which, k] = v
        else:
            out[i, 0, k] = out[i, 1, k] = v
    return out
