"""The culling decisions of the march, one by one, against binary64 geometry ("Direct tests of the culling
bounds").  rm_selftest_cull_rays / _pixels / _waves run the device functions of a draw -- cull_build_v5 and ray_misses_scene_v5,
pixel_misses_scene_v5, ray_misses_by_bounds_v5, wave_cull_lattice, wave_cull_blend -- with the launch a draw would fill; the
reference is tests/cull_ref.py (closest approaches, zones, scene infima), tests/scene_f64.py and, where the kernels compare
binary32 values, oracle/rm_oracle_np.py.  Every assertion is one-sided: a decision that culls must be RIGHT; how often the
kernels cull is the benchmark's business.  Inputs sit on the decision boundaries (rays that pass a zone at 0.5 .. 10 times its
size, directions with components 0, 1e-20 and subnormal, origins inside, on and behind, scenes 1e3 and 1e6 from the origin,
waves whose reach ends within 1e-5 of a unit's sphere), and every family must see both verdicts."""
import ctypes as C
import math

import numpy as np
import pytest

import cull_ref as R
import scene_f64
import scenes
from oracle import rm_oracle_np as onp
from ray_marching_amd import _ffi, renderer
from test_cull_tables_cpu import KIND_TO_OP, N_PARAMS, decode
from test_gpu_cull_differential import random_program

pytestmark = pytest.mark.gpu

F = np.float32
S_LIST = (0.5, 0.9, 0.99, 1.0, 1.01, 1.1, 2.0, 10.0)
MIN_DISTS = (-1.0, 0.0, 0.002, 0.01, 0.15, 5.0)
# How far the device's zone may lie inside the real one.  cull_margin adds up a dozen positive binary32 terms: its own relative
# rounding is below 16 * 2^-24.  The zone's faces (c + h + M) - ro and the cones' m = c - ro are three binary32 operations on
# coordinates of magnitude at most `scale`, each off by at most 2^-24 scale -- and M >= 1e-4 scale, which is what that term of M
# is for: 3 * 2^-24 * 1e4 M = 1.8e-3 M.  Together below 2e-3 of M.
M_ROUNDING = 3.0 * 2.0 ** -24 * 1.0e4 + 16.0 * 2.0 ** -24
assert M_ROUNDING < 2.0e-3


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(8192)
    yield r
    r.close()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def probe_rays(res, ro, dirs):
    ro, dirs = np.ascontiguousarray(ro, dtype=F), np.ascontiguousarray(dirs, dtype=F)
    flags, bound = np.zeros(len(dirs), dtype=np.uint32), np.zeros(len(dirs), dtype=F)
    res._check(res._L.rm_selftest_cull_rays(res._h, _ptr(ro), _ptr(dirs), len(dirs), _ptr(flags), _ptr(bound)))
    return flags, bound


def probe_pixels(res, W, H, xy):
    xy = np.ascontiguousarray(xy, dtype=np.uint32)
    out = np.zeros((len(xy), 8), dtype=F)
    res._check(res._L.rm_selftest_cull_pixels(res._h, W, H, _ptr(xy), len(xy), _ptr(out)))
    return out


def probe_waves(res, ro, pos, thr, live, extra_margin=0.0):
    """pos (n, 64, 3), thr (n, 64), live (n,) uint64 -> masks (n,) uint64"""
    n = len(pos)
    p = np.ascontiguousarray(np.transpose(np.asarray(pos, dtype=F), (0, 2, 1)))       # [wave][k][lane]
    thr, live, ro = np.ascontiguousarray(thr, dtype=F), np.ascontiguousarray(live, dtype=np.uint64), np.ascontiguousarray(ro, dtype=F)
    out = np.zeros(n, dtype=np.uint64)
    res._check(res._L.rm_selftest_cull_waves(res._h, _ptr(ro), _ptr(p), _ptr(thr), _ptr(live), n, C.c_float(extra_margin), _ptr(out)))
    return out


def set_case(res, cc, w, min_dist, cull=1):
    res.set_option(_ffi.RM_OPT_CULL, cull)
    res.set_limits((float(min_dist), 100.0, 64))
    res.set_program(cc, w)


# ---- programs -------------------------------------------------------------------------------------------------------------------
def _shift(cmds, off):
    out = []
    for op, a in cmds:
        a = list(a)
        if op in (0, 1, 10):
            a[:3] = [a[0] + off[0], a[1] + off[1], a[2] + off[2]]
        out.append((op, a))
    return out


def ray_programs(oracle):
    """[(name, cmd_count, words, scene centre)]: single leaves (as the Intersection of a leaf with itself, so that the walk on
    lower bounds applies and its bound is the leaf's), lattice programs with subtracted leaves, blending chains, every
    extension node, transforms; at the origin and 1e3 and 1e6 from it."""
    sph, box, cyl = (0, [0.2, -0.1, 0.3, 0.5]), (1, [0.2, -0.1, 0.3, 0.6, 0.2, 0.9]), (10, [0.2, -0.1, 0.3, 0.4, 0.8])
    out = []
    for name, leaf, off in (("sphere", sph, 0.0), ("box", box, 0.0), ("cylinder", cyl, 0.0), ("box at 1e3", box, 1e3), ("sphere at 1e3", sph, 1e3),
                            ("cylinder at 1e6", cyl, 1e6), ("flat box", (1, [0.2, -0.1, 0.3, 0.6, 0.0, 0.9]), 0.0),
                            ("sphere r<0", (0, [0.2, -0.1, 0.3, -0.25]), 0.0)):
        cmds = _shift([leaf, leaf, (102, [])], (off, -off, off))
        out.append((name, *R.words_of(*cmds), np.array(cmds[0][1][:3])))
    blend = [(0, [-0.6, 0.0, 0.0, 0.5]), (1, [0.7, 0.1, 0.0, 0.4, 0.3, 0.5]), (110, [0.3]), (10, [0.0, 0.9, 0.4, 0.3, 0.4]), (110, [0.05]),
             (0, [0.5, 0.2, 0.3, 0.35]), (101, []), (1, [-0.2, -0.8, 0.2, 0.9, 0.1, 0.9]), (100, [])]
    out.append(("blend chain", *R.words_of(*blend), np.zeros(3)))
    out.append(("blend chain at 1e3", *R.words_of(*_shift(blend, (1e3, 1e3, -1e3))), np.array([1e3, 1e3, -1e3])))
    for name in ("g8", "g8x", "g32s", "ext_mix", "xform_mix"):
        cc, w = oracle.serialize(*{**scenes.SCENES, **scenes.EXT_SCENES}[name]())
        out.append((name, cc, np.asarray(w, dtype=np.uint32), np.zeros(3)))
    for seed in (1,):
        cc, w = oracle.serialize(*random_program(np.random.default_rng(77000 + seed)))
        out.append(("cull chain %d" % seed, cc, np.asarray(w, dtype=np.uint32), np.zeros(3)))
    return out


def table_zones(d, ro, min_dist):
    """The zones of the program's table entries for camera position ro (binary32 values widened), M lowered by M_ROUNDING."""
    slack = float(F(d["smooth_slack"]))
    zones = []
    for r in d["rec"]:
        if r["kind"] not in (1, 2, 3) or r["nocull"]:
            continue
        if d["has_xforms"]:
            b = d["bounds"][r["slot"]]
            zones.append(R.zone(R.SPHERE, b, ro, min_dist, slack, shrink=M_ROUNDING))
        else:
            zones.append(R.zone(KIND_TO_OP[r["kind"]], r["p"][:N_PARAMS[r["kind"]]], ro, min_dist, slack, shrink=M_ROUNDING))
    return zones


def _perp(v, rng):
    t = np.cross(v, rng.normal(size=3))
    return t / np.linalg.norm(t)


def origins_for(d, centre, rng, min_dist):
    """Camera positions for one program: on a tangent line of a zone's face, edge and corner (and a sphere's surface), at a
    primitive's centre, inside its zone, on its boundary, 1e3 away, and behind it."""
    zones = table_zones(d, centre, min_dist)
    out = [centre + np.array([0.0, 0.0, 5.0]), centre + np.array([1e3, -2e2, 3e2])]
    for k, z in enumerate(zones[:2]):
        c, ext = z[1], (np.full(3, z[2]) if z[0] == "ball" else z[2])
        for f in ((1, 0, 0), (0, 1, 1), (1, -1, 1)):
            f = np.array(f, dtype=float)
            f = f / np.linalg.norm(f) * ext[0] if z[0] == "ball" else f * ext
            out.append(c + f - 3.0 * _perp(f, rng))                       # on the supporting plane at that feature
        if k == 0:
            out += [c.copy(), c + 0.5 * ext * np.array([1.0, 0.0, 0.0]), c + ext * np.array([0.0, 1.0, 0.0]), c - 4.0 * np.array([ext[0], 0.0, 0.0])]
    return [np.asarray(o, dtype=F) for o in out]


def directions_for(d, ro, rng, min_dist, n=1024):
    """Directions from ro: towards every zone's features scaled by S_LIST (a ray through c + s f passes the zone at s times its size
    when ro lies on the supporting plane at f), tangents to the zones' spheres scaled by S_LIST, away from the primitives,
    axis-parallel with components exactly 0, 1e-20 and subnormal; lengths 1e-3, 1 and 1e3."""
    ro = ro.astype(np.float64)
    zones = table_zones(d, ro, min_dist)
    dirs, special = [], []
    for z in zones[:6]:
        c, ext = z[1], (np.full(3, z[2]) if z[0] == "ball" else z[2])
        m = c - ro
        dist = np.linalg.norm(m)
        feats = [(1, 0, 0), (0, -1, 0), (0, 0, 1), (1, 1, 0), (0, 1, -1), (1, 1, 1), (-1, 1, -1)]
        for f in feats:
            f = np.array(f, dtype=float)
            f = f / np.linalg.norm(f) * ext[0] if z[0] == "ball" else f * ext
            t = _perp(f, rng)
            for s in S_LIST:
                dirs.append((c + s * f + 2.0 * t) - ro)
        Rz = float(np.linalg.norm(ext)) if z[0] == "box" else float(ext[0])
        if dist > 0.0:
            for s in S_LIST:                                               # tangent to the sphere of radius s Rz around c
                sin = s * Rz / dist
                if sin < 1.0:
                    dirs.append(math.sqrt(1.0 - sin * sin) * m / dist + sin * _perp(m, rng))
            special.append(-m)                                             # pointing away
    for ax in range(3):
        for tiny in (0.0, 1e-20, -1e-20, 1e-42):
            v = np.full(3, tiny)
            v[ax] = 1.0
            special += [v, -v]
    dirs, special = np.array(dirs).reshape(-1, 3), np.array(special)
    aimed = dirs[rng.permutation(len(dirs))[:max(n - len(special) - 8, 0)]]       # (all of them when there is room)
    dirs = np.concatenate([special, aimed, rng.normal(size=(8, 3))])
    dirs = dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * rng.choice([1e-3, 1.0, 1e3], size=(len(dirs), 1))
    return dirs.astype(F)


# ---- rays -----------------------------------------------------------------------------------------------------------------------
def check_rays(name, cc, w, d, ro, dirs, flags, bound, min_dist, stats):
    """The two ray assertions for one probe call; `stats` collects verdict counts and the smallest headrooms."""
    o64, d64 = ro.astype(np.float64), dirs.astype(np.float64)
    ok = np.linalg.norm(d64, axis=1) > 0.0
    clear, usable, walk, by_bounds = (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0
    assert not np.any(clear & ~usable) and not np.any(by_bounds & ~walk), name
    assert not np.any(clear[~ok]), name
    scale = d["scene_scale"] + np.abs(o64).sum()
    if clear.any():
        idx = np.flatnonzero(clear & ok)
        for z in table_zones(d, o64, min_dist):
            hit = R.meets_zone(z, o64, d64[idx])
            assert not hit.any(), "%s: ray from %s along %s is reported clear but meets the zone %s (min_dist %g)" % (
                name, ro.tolist(), dirs[idx[np.argmax(hit)]].tolist(), z, min_dist)
    stats["clear"] += int(clear.sum())
    stats["not clear"] += int((usable & ~clear).sum())
    if walk.any():
        assert walk[ok].all() and not np.isnan(bound[ok]).any(), name
        inf, t = R.scene_infimum(cc, w, o64, d64[ok], grid=64, refine=2, iters=16)
        b = bound[ok].astype(np.float64)
        k = int(np.argmax(b - inf))
        assert np.all(b <= inf), "%s: the bound %.9g of the ray from %s along %s exceeds the scene's value %.9g at t = %.9g" % (
            name, b[k], ro.tolist(), dirs[ok][k].tolist(), inf[k], t[k])
        cleared = by_bounds[ok]
        assert np.all(inf[cleared] > max(min_dist, 0.0)), name
        stats["walk clear"] += int(cleared.sum())
        stats["walk not clear"] += int((~cleared).sum())
        finite = np.isfinite(inf) & (b > -1e37)
        if finite.any():
            stats["bound headroom"] = min(stats["bound headroom"], float(((inf - b)[finite] / scale).min()))


@pytest.mark.parametrize("part", ["single leaves", "programs"])
def test_table_verdicts_and_lower_bounds_of_rays(res, oracle, part):
    progs = [p for k, p in enumerate(ray_programs(oracle)) if (k < 8) == (part == "single leaves")]
    stats = {"clear": 0, "not clear": 0, "walk clear": 0, "walk not clear": 0, "bound headroom": math.inf}
    rng = np.random.default_rng(51)
    n_walk = n_leaf_checks = 0
    for k, (name, cc, w, centre) in enumerate(progs):
        d = decode(cc, w)
        min_dist = MIN_DISTS[k % len(MIN_DISTS)]
        set_case(res, cc, w, min_dist)
        origins = origins_for(d, centre, rng, min_dist)
        per = max(64, 1024 // len(origins))
        for ro in origins:
            dirs = directions_for(d, ro, rng, min_dist, per)
            flags, bound = probe_rays(res, ro, dirs)
            n_walk += int((flags & 4).any())
            check_rays(name, cc, w, d, ro, dirs, flags, bound, min_dist, stats)
            if len(d["rec"]) == 2 and d["rec"][1]["mode"] == 3 and (flags & 4).all():     # the Intersection of a leaf with itself
                r0 = d["rec"][0]
                leaf_inf, _ = R.closest_approach(KIND_TO_OP[r0["kind"]], r0["p"][:N_PARAMS[r0["kind"]]], ro.astype(np.float64), dirs.astype(np.float64))
                assert np.all(bound.astype(np.float64) <= leaf_inf), (name, ro.tolist(), float((bound - leaf_inf).max()))
                n_leaf_checks += 1
    print("rays: %s" % stats)
    assert stats["clear"] > 100 and stats["not clear"] > 100 and stats["walk clear"] > 100 and stats["walk not clear"] > 100, stats
    assert n_walk > 20
    assert part != "single leaves" or n_leaf_checks >= 8 * 8


def test_rays_without_tables(res, oracle):
    """Culling switched off, a vetoed program and a Plane: no verdict from the tables; the Plane leaves the walk on lower bounds."""
    dirs = np.random.default_rng(52).normal(size=(130, 3)).astype(F)
    ro = np.array([0.0, 1.0, 5.0], dtype=F)
    cc, w = oracle.serialize(*scenes.g8())
    set_case(res, cc, w, 0.01, cull=0)
    flags, bound = probe_rays(res, ro, dirs)
    assert np.all(flags == 0) and np.isnan(bound).all()
    set_case(res, cc, w, 0.01, cull=1)
    assert (probe_rays(res, ro, dirs)[0] & 1).any()
    for prog in (R.words_of((204, [0.0]), (0, [0, 0, 0, 1.0]), (205, [])),                       # Scale by 0: cull_veto
                 R.words_of((1, [0, 0, 0, 0.5, math.nan, 0.5]), (0, [2, 0, 0, 0.5]), (100, []))):   # a box that is an infinite column
        set_case(res, *prog, 0.01)
        flags, bound = probe_rays(res, ro, dirs)
        assert np.all(flags == 0), prog
    set_case(res, *R.words_of((0, [0, 0, 0, 1.0]), (0, [math.inf, 0, 0, 1.0]), (100, [])), 0.01)  # the device's own veto (bit 0)
    flags, _ = probe_rays(res, ro, dirs)
    assert np.all((flags & 0xF) == 0) and np.all((flags >> 8) == 1)
    cc, w = R.words_of((0, [0, 0.5, 0, 1.0]), (2, [0.0, 1.0, 0.0, 1.5]), (100, []))                # a floor plane under a sphere
    set_case(res, cc, w, 0.01)
    flags, bound = probe_rays(res, ro, dirs)
    assert np.all((flags & 3) == 0) and np.all((flags >> 8) == 2) and np.all(flags & 4)
    up = dirs[:, 1] > 0.3
    assert (flags[up] & 8).any() and not (flags[dirs[:, 1] < -0.3] & 8).any()
    check_rays("plane", cc, w, decode(cc, w), ro, dirs, flags, bound, 0.01, {"clear": 0, "not clear": 0, "walk clear": 0, "walk not clear": 0,
                                                                               "bound headroom": math.inf})
    res.set_option(_ffi.RM_OPT_CULL, 1)


# ---- pixels ---------------------------------------------------------------------------------------------------------------------
def test_pixel_cones_and_verdicts(res, oracle):
    W, H = 48, 32
    progs = [p for p in ray_programs(oracle) if p[0] in ("box", "cylinder", "sphere at 1e3", "blend chain", "blend chain at 1e3", "g8", "g32s",
                                                         "ext_mix", "xform_mix", "cull chain 1", "cull chain 4")]
    rng = np.random.default_rng(53)
    stats = {"clear": 0, "not clear": 0, "walk clear": 0, "walk not clear": 0, "cone headroom": math.inf, "bound headroom": math.inf}
    for k, (name, cc, w, centre) in enumerate(progs):
        d = decode(cc, w)
        min_dist = MIN_DISTS[(k + 2) % len(MIN_DISTS)]
        set_case(res, cc, w, min_dist)
        events = [(1, float(rng.uniform(-300, 300)), float(rng.uniform(-100, 100))), (2, float(rng.uniform(-40, 100)), 0.0)]
        u, *_ = oracle.orbit_uniforms((float(W), float(H)), target=tuple(float(x) for x in centre), events=events)
        res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
        rays = np.stack([res.camera_rays(W, H, sample=s) for s in range(16)], axis=1)             # (W H, 16, 6)
        ro = rays[0, 0, :3]
        assert np.all(rays[:, :, :3] == ro)
        zones = table_zones(d, ro.astype(np.float64), min_dist)
        # the 256 pixels: those whose corner rays disagree about some zone (its silhouette), then random ones
        o64 = ro.astype(np.float64)
        meets = np.zeros((W * H, 16), dtype=bool)
        for z in zones:
            meets |= R.meets_zone(z, o64, rays[:, :, 3:].reshape(-1, 3).astype(np.float64)).reshape(W * H, 16)
        edge = np.flatnonzero(meets.any(axis=1) != meets.all(axis=1))
        near = np.flatnonzero(~meets.any(axis=1))
        pick = np.unique(np.concatenate([edge[:96], rng.choice(near, min(len(near), 120), replace=False) if len(near) else near,
                                         rng.integers(0, W * H, 40)]))[:256]
        xy = np.stack([pick % W, pick // W], axis=1)
        out = probe_pixels(res, W, H, xy)
        flags = out[:, 5].view(np.uint32)
        clear, usable, walk, by_bounds = (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0
        c, rho = out[:, :3].astype(np.float64), out[:, 3].astype(np.float64)
        e = rays[pick][:, :, 3:].astype(np.float64)
        assert not np.isnan(rho).any(), name                                     # (an ordinary camera: every pixel has a cone)
        gap = rho[:, None] - np.linalg.norm(e - c[:, None, :], axis=2)
        assert gap.min() >= 0.0, "%s: a sample direction lies %.3g outside its pixel's cone" % (name, -gap.min())
        stats["cone headroom"] = min(stats["cone headroom"], float(gap.min()))
        assert not np.any(clear & ~usable) and not np.any(by_bounds & ~walk), name
        assert not meets[pick][clear].any(), "%s: a pixel is reported clear but one of its sixteen rays meets a zone" % name
        stats["clear"] += int(clear.sum())
        stats["not clear"] += int((usable & ~clear).sum())
        if walk.any():
            idx = np.flatnonzero(walk)
            inf, _ = R.scene_infimum(cc, w, o64, e[idx].reshape(-1, 3), grid=64, refine=2, iters=16)
            inf = inf.reshape(len(idx), 16).min(axis=1)
            b = out[idx, 4].astype(np.float64)
            assert not np.isnan(b).any()
            assert np.all(b <= inf), (name, float((b - inf).max()))
            assert np.all(inf[by_bounds[idx]] > max(min_dist, 0.0)), name
            stats["walk clear"] += int(by_bounds.sum())
            stats["walk not clear"] += int((walk & ~by_bounds).sum())
            fin = b > -1e37
            if fin.any():
                stats["bound headroom"] = min(stats["bound headroom"], float(((inf - b)[fin] / (d["scene_scale"] + np.abs(o64).sum())).min()))
    print("pixels: %s" % stats)
    assert stats["clear"] > 100 and stats["not clear"] > 100 and stats["walk clear"] > 50 and stats["walk not clear"] > 50, stats


def test_pixel_bound_of_a_long_box_seen_end_on(res, oracle):
    """The far end of a long thin box lies |m| + |h| from the camera, and a sample ray strays from the pixel's centre ray by rho times
    that distance there: a ray grazing the far end is where the bounding radius in the inflation rho (|m| + R + max(c, 0)) of the
    CONE walk is needed.  Pixels around the far end's silhouette; both walk verdicts must occur."""
    W, H = 48, 32
    u, pos, *_ = oracle.orbit_uniforms((float(W), float(H)))
    axis = int(np.argmax(np.abs(pos)))                       # the camera looks down this axis at the origin
    h = np.full(3, 0.05)
    h[axis] = 3.0
    c = np.zeros(3)
    c[(axis + 1) % 3] = 0.3
    c[axis] = -1.0 * np.sign(pos[axis])                      # centre 6 from the camera, far end 9
    leaf = (1, c.tolist() + h.tolist())
    cc, w = R.words_of(leaf, leaf, (102, []))
    d = decode(cc, w)
    assert d["bound_walk"] == 1
    seen = {"clear": 0, "not clear": 0}
    for min_dist in (0.002, 0.15):
        set_case(res, cc, w, min_dist)
        res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
        rays = np.stack([res.camera_rays(W, H, sample=k) for k in range(16)], axis=1)
        o64 = rays[0, 0, :3].astype(np.float64)
        centre = res.camera_rays(W, H)[:, 3:].astype(np.float64)
        near, _ = R.closest_approach(R.BOX, np.array(leaf[1]), o64, centre)
        pick = np.argsort(np.abs(near - 0.05))[:256]         # the 256 pixels whose centre rays pass closest to 0.05 from the box
        out = probe_pixels(res, W, H, np.stack([pick % W, pick // W], axis=1))
        flags = out[:, 5].view(np.uint32)
        assert np.all(flags & 4), "the walk on lower bounds applies to every pixel"
        e = rays[pick][:, :, 3:].astype(np.float64)
        inf, _ = R.closest_approach(R.BOX, np.array(leaf[1]), o64, e.reshape(-1, 3))
        inf = inf.reshape(len(pick), 16).min(axis=1)
        b = out[:, 4].astype(np.float64)
        k = int(np.argmax(b - inf))
        assert np.all(b <= inf), "pixel %s: the bound %.9g over its cone exceeds the closest approach %.9g of one of its rays" % (
            (int(pick[k] % W), int(pick[k] // W)), b[k], inf[k])
        by_bounds = (flags & 8) != 0
        assert np.all(inf[by_bounds] > max(min_dist, 0.0))
        seen["clear"] += int(by_bounds.sum())
        seen["not clear"] += int((~by_bounds).sum())
        print("long box, min_dist %g: smallest (closest approach - bound) %.3g, rho %.3g" % (min_dist, float((inf - b).min()), float(out[:, 3].max())))
    assert seen["clear"] > 20 and seen["not clear"] > 20, seen


def test_pixels_without_a_usable_cone_are_never_clear(res, oracle):
    """rho = NaN never comes with a clear verdict: pixels too wide for the cone argument (a 4 x 3 frame: rho >= 0.05) and a
    projection that gives NaN directions."""
    cc, w = oracle.serialize(*scenes.g32s())
    set_case(res, cc, w, 0.01)
    u, *_ = oracle.orbit_uniforms((4.0, 3.0), events=[(1, 35.0, -25.0)])
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    xy = np.array([[x, y] for y in range(3) for x in range(4)], dtype=np.uint32)
    out = probe_pixels(res, 4, 3, xy)
    assert np.isnan(out[:, 3]).all() and np.all((out[:, 5].view(np.uint32) & 9) == 0) and np.isnan(out[:, 4]).all()
    bad = _ffi.Uniforms.from_buffer_copy(bytes(u))
    for k in range(16):
        bad.inv_proj[k] = math.nan
    res.set_uniforms(bad)
    out = probe_pixels(res, 4, 3, xy)
    assert np.isnan(out[:, 3]).all() and np.all((out[:, 5].view(np.uint32) & 9) == 0)
    # and the same pixels of a frame with a usable cone do get verdicts (the guard above is not vacuous)
    u, *_ = oracle.orbit_uniforms((48.0, 32.0), events=[(1, 35.0, -25.0)])
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    out = probe_pixels(res, 48, 32, xy)
    assert not np.isnan(out[:, 3]).any() and (out[:, 5].view(np.uint32) & 9).any()


# ---- waves: lattice programs ---------------------------------------------------------------------------------------------------
def _leaf_values(d, unit, pts):
    """The value of the unit's leaf at pts (n, 3) binary32: (binary64, binary32 widened)."""
    r = d["rec"][unit["first"]]
    prog = R.words_of((KIND_TO_OP[r["kind"]], r["p"][:N_PARAMS[r["kind"]]]))
    with np.errstate(all="ignore"):
        v32 = onp.map_scene(*prog, 100.0, pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()).astype(np.float64)
    return scene_f64.map_scene(*prog, 100.0, pts), v32


def _lattice_waves(d, rng, n_waves):
    """Positions spread over 1e-4 .. 10 around a common point; thresholds so that the wave's reach S = max (|p_l - p*| + thr_l)
    ends within 1e-5 of a unit's outer sphere (|p* - c| - R = S (1 +- 1e-5)) in three waves of four, random in the others."""
    units = [u for u in d["units"] if np.isfinite(u["p"][3])]
    cs = np.array([u["p"][:3] for u in units])
    pos = np.zeros((n_waves, 64, 3), dtype=F)
    thr = np.zeros((n_waves, 64), dtype=F)
    live = np.zeros(n_waves, dtype=np.uint64)
    for wv in range(n_waves):
        spread = 10.0 ** rng.uniform(-4, 1)
        p0 = cs[rng.integers(len(cs))] + rng.normal(size=3) * rng.choice([0.3, 1.5, 6.0])
        p = (p0 + rng.normal(size=(64, 3)) * spread * rng.uniform(0, 1, (64, 1))).astype(F)
        mask = rng.integers(0, 2 ** 63, dtype=np.uint64) | (rng.integers(0, 2, dtype=np.uint64) << np.uint64(63))
        if wv % 5 == 0:
            mask = np.uint64(0xFFFFFFFFFFFFFFFF)
        if mask == 0:
            mask = np.uint64(1) << np.uint64(17)
        lanes = np.array([i for i in range(64) if (int(mask) >> i) & 1])
        star = p[lanes[0]].astype(np.float64)
        reach = np.linalg.norm(p.astype(np.float64) - star, axis=1)
        t = rng.uniform(0, 1, 64) * rng.choice([1e-3, 0.1, 2.0])
        if wv % 4 != 3:
            u = units[rng.integers(len(units))]
            gap = np.linalg.norm(star - u["p"][:3]) - u["p"][3]
            S = gap * (1.0 + rng.choice([-1e-5, 1e-5, -1e-3, 1e-3]))
            if S > reach[lanes].max():
                t = np.maximum(S - reach, 0.0) * np.where(rng.random(64) < 0.3, 1.0, rng.uniform(0, 1, 64))
                t[lanes[-1]] = S - reach[lanes[-1]]
        pos[wv], thr[wv], live[wv] = p, t.astype(F), mask
    return pos, thr, live


def test_lattice_masks_skip_only_units_beyond_every_live_lanes_threshold(res, oracle):
    progs = []
    for name in ("g32", "g64", "g32_balanced", "g8x"):
        cc, w = oracle.serialize(*{**scenes.SCENES, **scenes.EXT_SCENES}[name]())
        progs.append((name, cc, np.asarray(w, dtype=np.uint32), np.zeros(3)))
    far = _shift([(0, [0.0, 0.0, 0.0, 0.5]), (1, [1.2, 0.1, 0.0, 0.4, 0.3, 0.5]), (100, []), (10, [0.0, 1.1, 0.4, 0.3, 0.4]), (100, []),
                  (0, [-1.0, 0.2, 0.3, 1e-4]), (100, []), (1, [0.3, -1.0, 0.2, 0.5, -0.1, 0.5]), (101, []), (0, [2.0, 2.0, 0.3, -0.3]), (100, [])], (1e3, -1e3, 1e3))
    progs.append(("lattice at 1e3", *R.words_of(*far), np.array([1e3, -1e3, 1e3])))
    progs.append(("a NaN leaf", *R.words_of((0, [0, 0, 0, 0.5]), (1, [1.5, 0, 0, 0.4, math.nan, 0.4]), (100, []), (0, [0, 2.0, 0, 0.5]), (100, [])), np.zeros(3)))
    rng = np.random.default_rng(54)
    skipped = kept = 0
    head = math.inf
    for name, cc, w, centre in progs:
        d = decode(cc, w)
        assert d["unit_mode"] == 1, name
        set_case(res, cc, w, 0.01)
        n_units = len(d["units"])
        valid = (1 << n_units) - 1
        pos, thr, live = _lattice_waves(d, rng, 256)
        ro = (centre + [0.0, 0.0, 5.0]).astype(F)
        masks = probe_waves(res, ro, pos, thr, live)
        assert np.all(masks & ~np.uint64(valid) == 0), name
        # dead lanes' garbage does not influence the mask
        pos2, thr2 = pos.copy(), thr.copy()
        dead = ((live[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)) == 0
        junk = rng.choice([np.nan, np.inf, -np.inf, 1e30, 0.0], size=pos.shape).astype(F)
        pos2[dead] = junk[dead]
        thr2[dead] = rng.choice([np.nan, np.inf, 1e30, -1.0], size=thr.shape).astype(F)[dead]
        assert np.array_equal(probe_waves(res, ro, pos2, thr2, live), masks), name
        lanes_live = ~dead
        scale = d["scene_scale"] + np.abs(ro).sum()
        for ui, u in enumerate(d["units"]):
            gone = ((masks >> np.uint64(ui)) & np.uint64(1)) == 0
            skipped += int(gone.sum())
            kept += int((~gone).sum())
            if not gone.any():
                continue
            assert np.isfinite(u["p"][3]), (name, ui)                     # a unit without a bound is never skipped
            sel = lanes_live[gone]
            pts = pos[gone][sel]
            t = thr[gone][sel].astype(np.float64)
            for label, v in zip(("binary64", "binary32"), _leaf_values(d, u, pts)):
                k = int(np.argmin(v - t))
                assert np.all(v > t), "%s unit %d: skipped, but its %s value %.9g at %s is not above the lane's threshold %.9g" % (
                    name, ui, label, v[k], pts[k].tolist(), t[k])
                head = min(head, float((v - t).min() / scale))
        # a NaN or +inf threshold, or a NaN position, in a live lane removes nothing
        for what in ("thr nan", "thr inf", "pos nan"):
            p3, t3 = pos[:64].copy(), thr[:64].copy()
            for wv in range(64):
                lane = int(rng.choice(np.flatnonzero(lanes_live[wv])))
                if what == "pos nan":
                    p3[wv, lane, int(rng.integers(3))] = np.nan
                else:
                    t3[wv, lane] = np.nan if what == "thr nan" else np.inf
            assert np.all(probe_waves(res, ro, p3, t3, live[:64]) == np.uint64(valid)), (name, what)
    print("lattice masks: %d skipped, %d kept, smallest (value - thr) / scale of a skipped unit %.3g" % (skipped, kept, head))
    assert skipped > 1000 and kept > 1000


def test_waves_probe_needs_units(res):
    set_case(res, *R.words_of((200, [1.0, 0.0, 0.0]), (0, [0, 0, 0, 1.0]), (201, [])), 0.01)      # a transform: no units
    with pytest.raises(_ffi.RmError) as e:
        probe_waves(res, np.zeros(3), np.zeros((1, 64, 3)), np.zeros((1, 64)), np.array([1], dtype=np.uint64))
    assert e.value.status == _ffi.RM_ERR_ARG


# ---- waves: blending chains ---------------------------------------------------------------------------------------------------
def _blend_chain(rng, centre):
    """A left-deep chain built step by step: (cmd_count, words, steps) with steps[j] = (kind, k, operand program); step 0 is the
    START leaf.  kind: "U" Union, "M" SmoothUnion(k), "S" Subtraction, "I" Intersection; an operand that is a sub-tree makes the
    step opaque ("O")."""
    def leaf():
        c = (centre + rng.uniform(-1.5, 1.5, 3)).tolist()
        r = rng.random()
        if r < 0.45:
            return (0, c + [float(rng.choice([rng.uniform(0.2, 0.7), 0.0, -0.2], p=[0.9, 0.05, 0.05]))])
        if r < 0.8:
            return (1, c + rng.uniform(0.1, 0.7, 3).tolist())
        return (10, c + [float(rng.uniform(0.1, 0.5)), float(rng.uniform(0.1, 0.8))])
    cmds = [leaf()]
    steps = [("START", 0.0, [cmds[0]])]
    for _ in range(int(rng.integers(6, 22))):
        sub = rng.random() < 0.12
        operand = [leaf(), leaf(), (100 if rng.random() < 0.6 else 101, [])] if sub else [leaf()]
        r = rng.random()
        if r < 0.5:
            k = float(rng.choice([rng.uniform(0.02, 0.6), 0.0, -0.3, 1e-6, 3.0], p=[0.7, 0.08, 0.07, 0.08, 0.07]))
            op, kind = (110, [k]), "M"
        elif r < 0.7:
            op, kind, k = (100, []), "U", 0.0
        elif r < 0.9:
            op, kind, k = (101, []), "S", 0.0
        else:
            op, kind, k = (102, []), "I", 0.0
        cmds += operand + [op]
        steps.append(("O" if sub else kind, k, operand, op))
    return (*R.words_of(*cmds), steps)


def _fold(kind, k, acc, v):
    """One operator of the chain in binary32, as oracle/rm_oracle_np.py applies it."""
    if kind in ("U", "M"):
        out = onp.fmin(acc, v)
        if kind == "M" and k > 0:
            kk = F(k)
            with np.errstate(invalid="ignore"):
                h = onp.fmax(kk - np.abs(acc - v), F(0)) / kk
            out = out - ((h * h) * kk) * F(0.25)
        return out.astype(F)
    if kind == "S":
        return onp.fmax(acc, -v)
    return onp.fmax(acc, v)


def _step_values(steps, pts):
    out = []
    for st in steps:
        with np.errstate(all="ignore"):
            out.append(onp.map_scene(*R.words_of(*st[2]), 100.0, pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()))
    return out


def _chain_values(steps, vals, upto=None):
    """Accumulator after every step (binary32), full chain."""
    acc, accs = vals[0], [vals[0]]
    for j in range(1, len(steps)):
        st = steps[j]
        kind = {100: "U", 101: "S", 102: "I", 110: "M"}[st[3][0]]
        acc = _fold(kind, st[1], acc, vals[j])
        accs.append(acc)
    return accs


def _rule_points(steps, rng, centre, n_steps=4, n_segments=16):
    """Points where a rule of wave_cull_blend is about to change its mind about some step u: v_u = acc + k (Union / SmoothUnion
    skipped), v_u = acc - k (restart), v_u = -acc (Subtraction), v_u = acc (Intersection), found by bisection along random
    segments, in binary64 arithmetic on the binary32 step values."""
    out = []
    for u in rng.choice(np.arange(1, len(steps)), min(n_steps, len(steps) - 1), replace=False):
        u = int(u)
        kind, k = steps[u][0], max(steps[u][1], 0.0)
        if kind == "O":
            continue
        a, b = centre + rng.uniform(-2.5, 2.5, (n_segments, 3)), centre + rng.uniform(-2.5, 2.5, (n_segments, 3))
        restart = rng.integers(0, 2, n_segments) == 1

        def g(t):
            p = (a + t[:, None] * (b - a)).astype(F)
            vals = _step_values(steps[:u + 1], p)
            acc = _chain_values(steps[:u], vals[:u])[-1].astype(np.float64)
            v = vals[u].astype(np.float64)
            if kind in ("U", "M"):
                return np.where(restart, v - (acc - k), v - (acc + k))
            return v + acc if kind == "S" else v - acc
        lo, hi = np.zeros(n_segments), np.ones(n_segments)
        glo, ghi = g(lo), g(hi)
        crossing = np.isfinite(glo) & np.isfinite(ghi) & (glo * ghi <= 0)
        for _ in range(24):
            mid = 0.5 * (lo + hi)
            gm = g(mid)
            same = gm * glo > 0
            lo, glo = np.where(same, mid, lo), np.where(same, gm, glo)
            hi = np.where(same, hi, mid)
        out += list((a + lo[:, None] * (b - a))[crossing])
    return out


def _check_blend_masks(res, name, cc, w, steps, ro, pos, live, counts):
    """For every live lane: the steps the mask names, from the leaf of the lowest named one, give the chain's value bit for bit."""
    n_waves = len(pos)
    lanes_live = ((live[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)) != 0
    flat = pos.reshape(-1, 3)
    vals = _step_values(steps, flat)
    full = _chain_values(steps, vals)[-1]
    with np.errstate(all="ignore"):
        assert full.tobytes() == onp.map_scene(cc, w, 100.0, flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 2].copy()).tobytes()
    for extra in (0.0, 0.01):
        masks = probe_waves(res, ro, pos, np.zeros((n_waves, 64), dtype=F), live, extra)
        assert np.all(masks >> np.uint64(len(steps)) == 0)
        bits = ((masks[:, None] >> np.arange(len(steps), dtype=np.uint64)[None, :]) & np.uint64(1)) != 0        # (wave, step)
        first = np.argmax(bits, axis=1)
        assert bits.any(axis=1).all()
        counts["restarts"] += int((first > 0).sum())
        counts["skipped"] += int((~bits).sum())
        counts["kept"] += int(bits.sum())
        per_lane = np.repeat(bits, 64, axis=0)                   # (wave * 64, step)
        start = np.repeat(first, 64)
        acc = np.zeros(len(flat), dtype=F)
        for j, st in enumerate(steps):
            begins = start == j
            acc = np.where(begins, vals[j], acc)
            if j == 0:
                continue
            kind = {100: "U", 101: "S", 102: "I", 110: "M"}[st[3][0]]
            assert not np.any(begins) or kind in ("U", "M")      # only a Union / SmoothUnion restarts the chain
            run = per_lane[:, j] & (start < j)
            acc = np.where(run, _fold(kind, st[1], acc, vals[j]), acc).astype(F)
        same = (acc.view(np.uint32) == full.view(np.uint32)) | (np.isnan(acc) & np.isnan(full))
        bad = np.flatnonzero(~same & lanes_live.reshape(-1))
        assert len(bad) == 0, "%s (extra margin %g): wave %d lane %d at %s: the named steps give %.9g, the chain %.9g; mask %x; words %s" % (
            name, extra, bad[0] // 64, bad[0] % 64, flat[bad[0]].tolist(), acc[bad[0]], full[bad[0]], int(masks[bad[0] // 64]), [int(x) for x in w])


def test_blend_masks_leave_the_chain_value_bit_identical(res):
    rng = np.random.default_rng(55)
    counts = {"skipped": 0, "kept": 0, "restarts": 0}
    n_progs = 0
    while n_progs < 12:
        centre = np.array([0.0, 0.0, 0.0]) if n_progs % 4 else np.array([1e3, 0.0, -1e3])
        cc, w, steps = _blend_chain(rng, centre)
        d = decode(cc, w)
        if d["unit_mode"] != 2:
            continue                                     # (no positive k drawn: a lattice program, not this family)
        n_progs += 1
        # the decoder sees the units the construction made
        want = {"START": 0, "U": 1, "M": 1, "S": 2, "I": 3, "O": 4}
        kinds = [want[st[0]] for st in steps]
        for j, st in enumerate(steps):                   # a SmoothUnion whose k is not positive still is a UM unit; its p[5] is 0
            if st[0] == "M":
                assert d["units"][j]["p"][5] == max(float(F(st[1])), 0.0)
        assert [u["kind"] for u in d["units"]] == kinds, (kinds, [u["kind"] for u in d["units"]])
        set_case(res, cc, w, 0.01)
        ro = (centre + [0.0, 0.0, 5.0]).astype(F)
        n_waves = 256
        anchors = _rule_points(steps, rng, centre)
        pos = np.zeros((n_waves, 64, 3), dtype=F)
        live = np.zeros(n_waves, dtype=np.uint64)
        for wv in range(n_waves):
            p0 = anchors[wv % len(anchors)] if anchors and wv % 4 != 3 else centre + rng.uniform(-3, 3, 3)
            spread = 10.0 ** rng.uniform(-4, 1 if wv % 4 == 3 else -1.5)
            pos[wv] = (p0 + rng.normal(size=(64, 3)) * spread * rng.uniform(0, 1, (64, 1))).astype(F)
            live[wv] = np.uint64(0xFFFFFFFFFFFFFFFF) if wv % 3 == 0 else (rng.integers(1, 2 ** 63, dtype=np.uint64) | np.uint64(1 << int(rng.integers(64))))
        _check_blend_masks(res, "chain %d" % n_progs, cc, w, steps, ro, pos, live, counts)
    print("blend masks: %s" % counts)
    assert counts["skipped"] > 1000 and counts["kept"] > 1000 and counts["restarts"] >= 1


def test_blend_masks_where_the_waves_radius_decides(res):
    """Spheres, whose outer and inner radii coincide, so that the rules' bounds L and H are as tight as the values: between two
    spheres a unit's value falls and the accumulator rises by the full distance a lane lies from p*, and a wave may skip the
    unit only if it is beyond a_hi + k by BOTH radii -- the one in L and the one in H.  Waves strung along the line between the
    centres, p* at 0.5 .. 3 wave radii beyond the point where the blend ends, rho from 1e-3 to 0.3, at the origin and 1e3 away."""
    counts = {"skipped": 0, "kept": 0, "restarts": 0}
    rng = np.random.default_rng(56)
    for off in (0.0, 1e3):
        for k in (0.2, 0.0):
            A, B, Cc = (0, [off - 1.0, 0.0, 0.0, 0.5]), (0, [off + 1.0, 0.0, 0.0, 0.5]), (0, [off, 6.0, 0.0, 0.5])
            second = (110, [k]) if k > 0 else (100, [])
            cmds = [A, B, second, Cc, (110, [0.1])]
            cc, w = R.words_of(*cmds)
            steps = [("START", 0.0, [A]), ("M" if k > 0 else "U", k, [B], second), ("M", 0.1, [Cc], (110, [0.1]))]
            d = decode(cc, w)
            assert d["unit_mode"] == 2 and [u["kind"] for u in d["units"]] == [0, 1, 1]
            set_case(res, cc, w, 0.01)
            # along the x axis between the centres: v_B - v_A - k = -2 (x - off) - k, zero at x0
            x0 = off - 0.5 * k
            pos = np.zeros((256, 64, 3), dtype=F)
            live = np.full(256, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
            for wv in range(256):
                rho = 10.0 ** rng.uniform(-3, -0.5) * (1.0 if off == 0.0 else 3.0)
                beyond = rng.choice([0.5, 0.9, 1.0, 1.1, 1.5, 1.9, 2.1, 3.0]) * rho       # v_B - (v_A + k) at p*, in wave radii
                xs = (x0 - 0.5 * beyond) + rho * np.concatenate([[0.0, 1.0], rng.uniform(0, 1, 62)])      # lane 0 is p*; lane 1 a radius towards B
                pos[wv, :, 0] = xs.astype(F)
                pos[wv, :, 1:] = (rng.normal(size=(64, 2)) * 1e-3 * rho).astype(F)
                pos[wv, 0, 1:] = 0.0
            _check_blend_masks(res, "spheres k=%g at %g" % (k, off), cc, w, steps, np.array([off, 0.0, 5.0], dtype=F), pos, live, counts)
    print("blend masks, tight spheres: %s" % counts)
    assert counts["skipped"] > 200 and counts["kept"] > 200
