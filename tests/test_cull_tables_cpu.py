"""The data the culling rules of the march read (ray-marching_amd/csrc/rm_decode.h), checked one claim at a time against binary64
geometry ("Direct tests of the culling bounds"): the unit records' outer and inner radii, the world-space
bounding spheres of transformed primitives, smooth_slack, scene_scale and the vetoes.  tests/cpp/cull_tables_probe.cpp prints
them; values come from tests/scene_f64.py (binary64) and oracle/rm_oracle_np.py (binary32: the kernels compare binary32 values).
Programs: the named scenes, the three generators of tests/fuzz_programs.py, the blending chains of
tests/test_gpu_cull_differential.py, and a list of degenerate leaves."""
import atexit
import json
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import cull_ref as R
import fuzz_programs
import scene_f64
import scenes
from oracle import rm_oracle_np as onp
from test_gpu_cull_differential import random_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = float("inf")
KIND_TO_OP = {1: R.SPHERE, 2: R.BOX, 3: R.CYLINDER, 4: R.PLANE}
N_PARAMS = {1: 4, 2: 6, 3: 5, 4: 4}
UNIT_START, UNIT_UM, UNIT_SUB, UNIT_INTER, UNIT_OPAQUE, UNIT_LEAF = range(6)
MAX_XFORM_DEPTH = 8
QUAT_VETO = 1.0e-4            # rm_decode.h: a quaternion whose squared norm is not within this of 1 vetoes culling

# ---- the probe ------------------------------------------------------------------------------------------------------------------
_PROBE = []


def _probe_exe():
    if not _PROBE:
        d = tempfile.mkdtemp(prefix="rm_cull_tables_probe_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "cull_tables_probe")
        b = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "cpp", "cull_tables_probe.cpp")], capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr[-3000:]
        _PROBE.append(exe)
    return _PROBE[0]


def _f(bits):
    return np.asarray(bits, dtype=np.uint32).view(F).astype(np.float64)


def decode_many(programs):
    """What the decoder makes of each (cmd_count, words): a dict with floats widened to binary64 (rc != 0: only "rc")."""
    text = "".join("%d %d\n%s\n" % (cc, len(w), " ".join(str(int(x)) for x in np.asarray(w, dtype=np.uint32))) for cc, w in programs)
    run = subprocess.run([_probe_exe()], input=text, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    out = [json.loads(line) for line in run.stdout.splitlines()]
    assert len(out) == len(programs)
    for d in out:
        if d["rc"] != 0:
            continue
        for key in ("unit_kmax", "scene_scale"):
            d[key] = float(_f([d[key]])[0])
        d["smooth_slack"] = float(np.array([d["smooth_slack"]], dtype=np.uint64).view(np.float64)[0])
        d["bounds"] = _f(d["bounds"]).reshape(-1, 4)
        d["units"] = [dict(kind=u[0], first=u[1], last=u[2], p=_f(u[3:9])) for u in d["units"]]
        d["rec"] = [dict(kind=r[0], mode=r[1], nocull=r[2], slot=r[3], unit=r[4], cmd=r[5], p=_f(r[6:12])) for r in d["rec"]]
    return out


def decode(cc, words):
    return decode_many([(cc, words)])[0]


# ---- the programs ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs(oracle):
    """[(name, cmd_count, words, decoded)]"""
    out = []
    named = {**scenes.SCENES, **scenes.EXT_SCENES, **scenes.MAT_SCENES, "right_deep6": lambda: scenes.right_deep(6)}
    for name, fn in named.items():
        cc, w = oracle.serialize(*fn())
        out.append((name, cc, np.asarray(w, dtype=np.uint32)))
    for cls in fuzz_programs.CLASSES:
        for seed in fuzz_programs.SEEDS:
            c = fuzz_programs.case(oracle, cls, seed)
            out.append(("%s %d" % (cls, seed), c.cc, c.words))
    for seed in range(16):
        cc, w = oracle.serialize(*random_program(np.random.default_rng(77000 + seed)))
        out.append(("cull chain %d" % seed, cc, np.asarray(w, dtype=np.uint32)))
    dec = decode_many([(cc, w) for _, cc, w in out])
    assert all(d["rc"] == 0 for d in dec)
    return [(n, cc, w, d) for (n, cc, w), d in zip(out, dec)]


DEGENERATE = [
    ("sphere r=0", (0, [0.5, -0.25, 1.0, 0.0])),
    ("sphere r<0", (0, [0.5, -0.25, 1.0, -0.75])),
    ("sphere r=1e-4", (0, [0.5, -0.25, 1.0, 1e-4])),
    ("sphere r=1e4", (0, [0.5, -0.25, 1.0, 1e4])),
    ("sphere at 1e3", (0, [1e3, -1e3, 1e3, 0.5])),
    ("sphere at 1e6", (0, [1e6, 1e6, -1e6, 0.5])),
    ("box h=0", (1, [0.5, -0.25, 1.0, 0.0, 0.0, 0.0])),
    ("box all h<0", (1, [0.5, -0.25, 1.0, -0.5, -0.25, -1.0])),
    ("box one h<0", (1, [0.5, -0.25, 1.0, 0.5, -0.25, 1.0])),
    ("box one h=0", (1, [0.5, -0.25, 1.0, 0.5, 0.0, 1.0])),
    ("box h=1e-4", (1, [0.5, -0.25, 1.0, 1e-4, 2e-4, 1e-4])),
    ("box h=1e4", (1, [0.5, -0.25, 1.0, 1e4, 1.0, 1e-4])),
    ("box at 1e3", (1, [1e3, -1e3, 1e3, 0.5, 0.25, 1.0])),
    ("box at 1e6", (1, [1e6, 1e6, -1e6, 0.5, 0.25, 1.0])),
    ("cylinder r=0", (10, [0.5, -0.25, 1.0, 0.0, 0.5])),
    ("cylinder hh=0", (10, [0.5, -0.25, 1.0, 0.5, 0.0])),
    ("cylinder r<0", (10, [0.5, -0.25, 1.0, -0.5, 0.5])),
    ("cylinder hh<0", (10, [0.5, -0.25, 1.0, 0.5, -0.5])),
    ("cylinder both<0", (10, [0.5, -0.25, 1.0, -0.25, -0.5])),
    ("cylinder r=1e-4", (10, [0.5, -0.25, 1.0, 1e-4, 1.0])),
    ("cylinder r=1e4", (10, [0.5, -0.25, 1.0, 1e4, 1.0])),
    ("cylinder at 1e3", (10, [1e3, -1e3, 1e3, 0.5, 0.25])),
    ("cylinder at 1e6", (10, [1e6, 1e6, -1e6, 0.5, 0.25])),
]
NOT_FINITE = [
    ("sphere r=NaN", (0, [0.5, -0.25, 1.0, math.nan])),
    ("sphere r=inf", (0, [0.5, -0.25, 1.0, INF])),
    ("sphere r=-inf", (0, [0.5, -0.25, 1.0, -INF])),
    ("sphere c=NaN", (0, [0.5, math.nan, 1.0, 0.5])),
    ("sphere c=inf", (0, [INF, -0.25, 1.0, 0.5])),
    ("box h=NaN", (1, [0.5, -0.25, 1.0, 0.5, math.nan, 1.0])),
    ("box h=inf", (1, [0.5, -0.25, 1.0, 0.5, 0.25, INF])),
    ("box c=-inf", (1, [0.5, -INF, 1.0, 0.5, 0.25, 1.0])),
    ("cylinder r=NaN", (10, [0.5, -0.25, 1.0, math.nan, 0.5])),
    ("cylinder hh=inf", (10, [0.5, -0.25, 1.0, 0.5, INF])),
    ("cylinder c=NaN", (10, [0.5, -0.25, math.nan, 0.5, 0.5])),
]
_NEIGHBOUR = (0, [3.0, 0.0, 0.0, 0.5])     # (a lattice program of two leaves: the degenerate one and a healthy sphere)


# ---- unit radii -----------------------------------------------------------------------------------------------------------------
_DIRS = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], dtype=np.float64)
_DIRS = np.concatenate([_DIRS / np.linalg.norm(_DIRS, axis=1, keepdims=True),
                        (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(np.random.default_rng(11).normal(size=(22, 3)))])


def unit_points(kind, a):
    """Binary32 points around leaf (kind, a): shells at radii 0 .. 100 R, the corners, edge midpoints and face centres of its
    bounding box (the rim and cap centres of a cylinder are among them), the axis of its smallest extent, the centre."""
    c = a[:3]
    ext = {1: np.full(3, a[3]), 2: a[3:6], 3: np.array([a[3], a[4], a[3]]) if kind == 3 else None}[kind]
    Rg = float(np.linalg.norm(np.maximum(ext, 0.0))) if kind != 1 else max(float(a[3]), 0.0)
    scale = Rg if Rg > 0.0 else max(float(np.abs(ext).max()), 1e-3)
    parts = [c[None, :]]
    for s in (1e-3, 0.25, 0.5, 0.9, 0.999, 1.0, 1.001, 1.1, 2.0, 10.0, 100.0):
        parts.append(c + s * scale * _DIRS)
    grid = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], dtype=np.float64)
    for s in (0.999, 1.0, 1.001):
        parts.append(c + s * grid * np.abs(ext))                   # corners, edge midpoints, face centres (and the centre)
    i = int(np.argmin(np.abs(ext)))
    ts = np.concatenate([np.linspace(-2.0, 2.0, 41) * max(abs(ext[i]), 1e-3), np.linspace(-2.0, 2.0, 9) * scale])
    parts.append(c + ts[:, None] * np.eye(3)[i])
    return np.concatenate(parts).astype(F)


# The radii are constants, and the rounding of a binary32 VALUE at distance D from the leaf grows with D (half an ulp of D for the
# square root alone): no constant absorbs it at 100 R.  The kernels therefore never compare against |q - c| itself: unit_bounds
# takes d 0.999998 on the outer side and d 1.000002 on the inner one, wave_cull_lattice 1.000004 on the squares.  The binary32
# value is held to the claim in that form; the binary64 value, which has no such rounding, to the claim as the decoder states it.
KERNEL_REL = 2.0e-6


def check_unit_radii(name, d):
    """value_u(q) >= |q - c| - p[3] and value_u(q) <= |q - c| - p[4] in binary64; for the binary32 value with |q - c| lowered /
    raised by the kernels' own KERNEL_REL.  Returns the smallest headrooms relative to 1 + |c|_1 + |size|_1 (outer, inner)."""
    head = [INF, INF]
    for ui, u in enumerate(d["units"]):
        if u["kind"] == UNIT_OPAQUE:
            assert u["p"][3] == INF and u["p"][4] == -INF, (name, ui)
            continue
        leaf = d["rec"][u["first"]]
        kind, a = leaf["kind"], leaf["p"][:N_PARAMS[leaf["kind"]]]
        assert kind in (1, 2, 3), (name, ui, kind)
        if not np.all(np.isfinite(a)):
            assert u["p"][3] == INF and u["p"][4] == -INF, (name, ui, a, u["p"])
            continue
        assert np.array_equal(u["p"][:3], a[:3]), (name, ui)
        assert np.isfinite(u["p"][3]) and np.isfinite(u["p"][4]) and u["p"][3] >= 0.0
        q = unit_points(kind, a)
        dist = np.linalg.norm(q.astype(np.float64) - a[:3], axis=1)
        cc1, w1 = R.words_of((KIND_TO_OP[kind], a))
        v64 = scene_f64.map_scene(cc1, w1, 100.0, q)
        with np.errstate(all="ignore"):
            v32 = onp.map_scene(cc1, w1, 100.0, q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy()).astype(np.float64)
        norm = 1.0 + np.abs(a).sum()
        for label, v, rel in (("binary64", v64, 0.0), ("binary32", v32, KERNEL_REL)):
            lo, hi = v - (dist * (1.0 - rel) - u["p"][3]), (dist * (1.0 + rel) - u["p"][4]) - v
            k = int(np.argmin(np.minimum(lo, hi)))
            assert lo.min() >= 0.0 and hi.min() >= 0.0, \
                "%s unit %d kind %d params %s, %s value at %s: value %.9g, |q - c| %.9g, outer %.9g inner %.9g" % (
                    name, ui, kind, a.tolist(), label, q[k].tolist(), v[k], dist[k], u["p"][3], u["p"][4])
            head = [min(head[0], lo.min() / norm), min(head[1], hi.min() / norm)]
    return head


def test_unit_radii_bound_the_leaf_from_both_sides(programs):
    seen = set()
    head = [INF, INF]
    for name, cc, w, d in programs:
        if d["units"]:
            seen.add(d["unit_mode"])
            h = check_unit_radii(name, d)
            head = [min(head[0], h[0]), min(head[1], h[1])]
            assert d["unit_kmax"] == max([0.0] + [u["p"][5] for u in d["units"]])
    assert seen == {1, 2}, "both lattice programs and blending chains must be among the programs"
    print("smallest headroom / (1 + |c|_1 + |size|_1): outer %.3g inner %.3g" % tuple(head))


@pytest.mark.parametrize("name,leaf", DEGENERATE, ids=[x[0] for x in DEGENERATE])
def test_unit_radii_of_degenerate_leaves(name, leaf):
    for prog in (R.words_of(leaf, _NEIGHBOUR, (100, [])), R.words_of(_NEIGHBOUR, leaf, (110, [0.25]))):     # lattice; blending chain
        d = decode(*prog)
        assert d["rc"] == 0 and len(d["units"]) == 2
        check_unit_radii(name, d)


@pytest.mark.parametrize("name,leaf", NOT_FINITE, ids=[x[0] for x in NOT_FINITE])
def test_leaves_that_are_not_finite_have_no_bound_at_all(name, leaf):
    for prog, at in ((R.words_of(leaf, _NEIGHBOUR, (100, [])), 0), (R.words_of(_NEIGHBOUR, leaf, (110, [0.25])), 1)):
        d = decode(*prog)
        assert d["rc"] == 0 and len(d["units"]) == 2
        u = d["units"][at]
        assert u["p"][3] == INF and u["p"][4] == -INF, (name, u)
        if any(math.isinf(x) for x in leaf[1]):      # an infinite scale: no float margin is derived from it, no walk on lower bounds
            assert d["scene_scale"] == INF and d["bound_walk"] == 0
        # a box or cylinder with a NaN size is an infinite slab or column (the NaN drops out of its maxima): nothing may be culled
        assert d["cull_veto"] == int(leaf[0] != 0 and any(math.isnan(x) for x in leaf[1][3:])), name
        h = d["units"][1 - at]
        assert np.isfinite(h["p"][3]) and np.isfinite(h["p"][4])


# ---- world-space bounding spheres ---------------------------------------------------------------------------------------------
def _near_unit_quaternion(rng, stretch):
    """A quaternion whose squared norm is 1 + stretch after rounding to binary32 (|stretch| below the veto threshold)."""
    q = rng.normal(size=4)
    q = (q / np.linalg.norm(q) * math.sqrt(1.0 + stretch)).astype(F)
    assert abs(float((q.astype(np.float64) ** 2).sum()) - 1.0) < QUAT_VETO
    return [float(x) for x in q]


def _scoped_leaf_programs():
    """Single leaves inside 1 .. 8 transform scopes: scale factors 1e-3 .. 1e3, quaternions just inside the veto threshold
    (squared norm 1 +- 0.99e-4) and exactly unit ones, translations up to 1e3, leaves on and far off their local origin."""
    rng = np.random.default_rng(21)
    leaves = [(0, [0.0, 0.0, 0.0, 0.5]), (0, [30.0, -20.0, 10.0, 0.01]), (1, [0.2, -0.1, 0.3, 0.6, 0.2, 0.9]), (1, [100.0, 0.0, 0.0, 0.05, 0.05, 0.05]),
              (10, [0.1, 0.2, -0.3, 0.4, 0.8]), (10, [-40.0, 25.0, 5.0, 0.1, 0.3]), (1, [0.5, 0.5, 0.5, -0.2, 0.3, 0.4]), (0, [1.0, 2.0, 3.0, -0.5])]
    out = []
    for depth in (1, 2, 3, 5, MAX_XFORM_DEPTH):
        for trial in range(8):
            leaf = leaves[(trial + depth) % len(leaves)]
            cmds, pops = [], []
            for level in range(depth):
                kind = (level + trial) % 3 if depth > 1 else trial % 3
                if kind == 0:
                    cmds.append((200, [float(x) for x in rng.uniform(-1, 1, 3) * rng.choice([1.0, 1e3])]))
                    pops.append((201, []))
                elif kind == 1:
                    cmds.append((202, _near_unit_quaternion(rng, float(rng.choice([0.99e-4, -0.99e-4, 0.0])))))
                    pops.append((203, []))
                else:
                    cmds.append((204, [float(rng.choice([1e-3, 0.03, 0.5, 1.0, 2.0, 40.0, 1e3]))]))
                    pops.append((205, []))
            out.append(("depth %d trial %d" % (depth, trial), R.words_of(*(cmds + [leaf] + pops[::-1]))))
    return out


# A quaternion q = s u (u unit, s^2 = 1 + e, |e| < 1e-4) maps v to v + s^2 (R_u v - v) = (1 - s^2) v + s^2 R_u v: a linear map
# whose stretch lies in [1 - 2 |e|, 1 + 2 |e|].  D nested scopes hold at most D such maps (translations and scales are exact
# similarities), so a world-space length shrinks by at most (1 - 2e-4)^D on its way to the leaf's own frame:
EPS = 1.0 - (1.0 - 2.0 * QUAT_VETO) ** MAX_XFORM_DEPTH        # 1.6e-3


def _shell(cc, w, c, radius):
    """Points at `radius` (and a hair more) from c: the fixed directions, and the directions in which the leaf lies from c --
    towards the lowest values of a cloud around c, where a misplaced centre shows first."""
    cloud = c + np.random.default_rng(3).normal(size=(400, 3)) * max(radius, 1e-6)
    best = cloud[np.argsort(scene_f64.map_scene(cc, w, 100.0, cloud))[:8]] - c
    dirs = np.concatenate([_DIRS, best / np.maximum(np.linalg.norm(best, axis=1, keepdims=True), 1e-300)])
    return c + radius * (1.0 + 1e-12) * dirs


def test_bounding_sphere_of_a_leaf_far_from_the_origin_of_a_slightly_non_unit_rotation():
    """Regression.  A quaternion of squared norm 1 + e (|e| < 1e-4 passes the veto) maps with (1 - |q|^2) I + |q|^2 R; the decoder
    places the centre with it, the evaluation goes back with the conjugate's map, and the two are not inverses: the leaf sits up
    to 4 |e| |c| from where the decoder put it.  With |c| = 37 and e = 0.99e-4 that is 0.015 for a sphere of radius 0.01: before
    the fix its whole surface lay outside its bounding sphere."""
    rng = np.random.default_rng(8)
    for e in (0.99e-4, -0.99e-4):
        for _ in range(6):
            cc, w = R.words_of((202, _near_unit_quaternion(rng, e)), (0, [30.0, -20.0, 10.0, 0.01]), (203, []))
            d = decode(cc, w)
            assert d["cull_veto"] == 0
            c, rho = d["bounds"][0, :3], d["bounds"][0, 3]
            pts = c + rho * (1.0 + 1e-12) * (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(4000, 3)))
            assert scene_f64.map_scene(cc, w, 100.0, pts).min() >= 0.0
            assert scene_f64.map_scene(cc, w, 100.0, _shell(cc, w, c, rho)).min() >= 0.0
            assert rho < 0.01 * 1.002 + 4.1e-4 * 37.5            # and the slack is what the derivation asks for, not more


def test_world_space_bounding_spheres_contain_their_leaf():
    """For the single leaf inside its scopes: every q with |q - c| >= rho + m has value(q) >= m (1 - EPS), m from 0 to a few scene
    scales -- the claim the miss tests need (value >= |q - c| - rho itself is not true far away under a non-unit quaternion)."""
    progs = _scoped_leaf_programs()
    decs = decode_many([p for _, p in progs])
    head = INF
    for (name, (cc, w)), d in zip(progs, decs):
        assert d["rc"] == 0 and d["has_xforms"] == 1 and d["cull_veto"] == 0 and len(d["bounds"]) == 1, (name, d)
        c, rho = d["bounds"][0, :3], d["bounds"][0, 3]
        assert np.all(np.isfinite(d["bounds"]))
        for m in (0.0, 1e-6 * rho, 1e-3 * rho, 0.1 * rho, rho, 0.01 * d["scene_scale"], d["scene_scale"], 3.0 * d["scene_scale"]):
            q = _shell(cc, w, c, rho + m)
            v = scene_f64.map_scene(cc, w, 100.0, q)
            k = int(np.argmin(v))
            assert v[k] >= m * (1.0 - EPS), "%s: value %.9g at %s, |q - c| = rho + m with rho %.9g m %.9g; program %s" % (
                name, v[k], q[k].tolist(), rho, m, [int(x) for x in w])
            head = min(head, (v[k] - m * (1.0 - EPS)) / d["scene_scale"])
    print("smallest headroom / scene_scale: %.3g" % head)


def test_bounding_spheres_of_the_programs_with_transforms(programs):
    """The same claim inside whole programs: the leaf alone in its scopes (the commands of the program that are not its scopes'
    are dropped) stays at least m away from every point m outside its sphere."""
    n = 0
    for name, cc, w, d in programs:
        if not d["has_xforms"] or d["cull_veto"]:
            continue
        cmds = R.commands(cc, w)
        raw = [(op, a) for op, a, _ in cmds if op != 300]          # (the records index the program without its tags)
        prims = [r for r in d["rec"] if r["kind"] in (1, 2, 3)]
        assert len(prims) == len(d["bounds"])
        for r in prims:
            # the scopes open at the leaf: walk the commands up to it
            open_scopes = []
            for op, a in raw[:r["cmd"]]:
                if op in (200, 202, 204):
                    open_scopes.append((op, a))
                elif op in (201, 203, 205):
                    open_scopes.pop()
            leaf = raw[r["cmd"]]
            assert leaf[0] == KIND_TO_OP[r["kind"]]
            prog = R.words_of(*(open_scopes + [leaf] + [(op + 1, []) for op, _ in open_scopes[::-1]]))
            c, rho = d["bounds"][r["slot"], :3], d["bounds"][r["slot"], 3]
            for m in (0.0, 0.1 * rho, d["scene_scale"]):
                v = scene_f64.map_scene(*prog, 100.0, _shell(*prog, c, rho + m))
                assert v.min() >= m * (1.0 - EPS), (name, r["cmd"], m, float(v.min()))
            n += 1
    assert n >= 10


# ---- blend slack, scene scale ----------------------------------------------------------------------------------------------------
def _without_blends(cc, w):
    """The same program with every SmoothUnion's k set to 0: the plain minimum."""
    w = np.array(w, dtype=np.uint32)
    at = 0
    for _ in range(cc):
        op = int(w[at])
        if op == 110:
            w[at + 1] = 0
        at += 1 + scene_f64._PARAMS[op]
    return w


def _near_surface_points(cc, w, rng, n=600):
    """Random points of the scene's neighbourhood and points pushed onto (and just off) its surface by a few Newton steps."""
    lo, hi = -4.0, 4.0
    p = rng.uniform(lo, hi, (n, 3))
    q = p.copy()
    for _ in range(6):
        v = scene_f64.map_scene(cc, w, 100.0, q)
        g = np.stack([(scene_f64.map_scene(cc, w, 100.0, q + 1e-5 * e) - scene_f64.map_scene(cc, w, 100.0, q - 1e-5 * e)) / 2e-5 for e in np.eye(3)], axis=1)
        gn = np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-3)
        q = q - np.clip(v, -2.0, 2.0)[:, None] * g / (gn * gn)
    q = q[np.all(np.isfinite(q), axis=1)]
    return np.concatenate([p, q, q + rng.normal(size=q.shape) * 0.05])


def test_smooth_slack_bounds_how_far_blends_pull_the_value_down(programs):
    rng = np.random.default_rng(31)
    n, worst = 0, INF
    for name, cc, w, d in programs:
        assert d["smooth_slack"] >= 0.0
        has_blend = any(op == 110 and a[0] > 0 for op, a, _ in R.commands(cc, w))
        assert (d["smooth_slack"] > 0.0) == has_blend, name
        if not has_blend:
            continue
        pts = _near_surface_points(cc, w, rng)
        blended, plain = scene_f64.map_scene(cc, w, 100.0, pts), scene_f64.map_scene(cc, _without_blends(cc, w), 100.0, pts)
        gap = blended - (plain - d["smooth_slack"])
        assert gap.min() >= -1e-12, (name, float(gap.min()), d["smooth_slack"])
        worst = min(worst, float(gap.min()) / d["scene_scale"])
        n += int((plain - blended).max() > 1e-3)       # some point lies well inside a blend zone
    assert n >= 8
    print("smallest (F - (F_min - smooth_slack)) / scene_scale: %.3g" % worst)


def test_scene_scale_covers_every_primitive_and_blend_radius(programs):
    extra = [("k = -7", *R.words_of((0, [0, 0, 0, 1.0]), (0, [1, 0, 0, 1.0]), (110, [-7.0]))),
             ("far box", *R.words_of((1, [1e3, -2e3, 5e2, 3.0, 4.0, 5.0]))), ("plane", *R.words_of((2, [0.0, 3.0, 0.0, -9.0])))]
    extra = [(n, cc, w, d) for (n, cc, w), d in zip(extra, decode_many([(cc, w) for _, cc, w in extra]))]
    for name, cc, w, d in list(programs) + extra:
        for op, a, _ in R.commands(cc, w):
            if op in (R.SPHERE, R.BOX, R.CYLINDER, R.PLANE):
                assert d["scene_scale"] >= 1.0 + float(np.abs(a).sum()), (name, op, a)
            elif op == 110:
                assert d["scene_scale"] >= 1.0 + abs(float(a[0])), (name, a)


# ---- vetoes ---------------------------------------------------------------------------------------------------------------------
_LEAF = (0, [0.25, 0.5, -0.5, 0.75])


def _scoped(push, leaf=_LEAF):
    return R.words_of(push, leaf, (push[0] + 1, []))


def test_transforms_that_are_no_finite_similarity_veto_culling():
    h = math.sqrt(0.5)
    bad = {
        "quaternion norm^2 = 1 + 1.1e-4": (202, [float(F(math.sqrt(1.00011))), 0.0, 0.0, 0.0]),
        "quaternion norm^2 = 1 - 1.1e-4": (202, [0.0, float(F(math.sqrt(0.99989))), 0.0, 0.0]),
        "quaternion 0": (202, [0.0, 0.0, 0.0, 0.0]),
        "quaternion NaN": (202, [h, math.nan, 0.0, h]),
        "quaternion inf": (202, [INF, 0.0, 0.0, 0.0]),
        "scale 0": (204, [0.0]), "scale -1": (204, [-1.0]), "scale NaN": (204, [math.nan]), "scale inf": (204, [INF]),
        "scale -0": (204, [-0.0]), "scale 1e30": (204, [1e30]),
        "translation NaN": (200, [0.0, math.nan, 0.0]), "translation inf": (200, [INF, 0.0, 0.0]), "translation -inf": (200, [0.0, 0.0, -INF]),
    }
    good = {
        "identity quaternion": (202, [1.0, 0.0, 0.0, 0.0]), "quarter turn": (202, [h, h, 0.0, 0.0]),
        "quaternion norm^2 = 1 + 0.9e-4": (202, [float(F(math.sqrt(1.00009))), 0.0, 0.0, 0.0]),
        "quaternion norm^2 = 1 - 0.9e-4": (202, [0.0, 0.0, float(F(math.sqrt(0.99991))), 0.0]),
        "scale 1e-3": (204, [1e-3]), "scale 1e3": (204, [1e3]), "scale 1e-30": (204, [1e-30]),
        "translation 1e6": (200, [1e6, -1e6, 1e6]), "translation 0": (200, [0.0, 0.0, 0.0]),
    }
    names = list(bad) + list(good)
    decs = decode_many([_scoped({**bad, **good}[n]) for n in names])
    for n, d in zip(names, decs):
        assert d["rc"] == 0, n
        assert d["cull_veto"] == (1 if n in bad else 0), n
    # the veto is the program's: one bad scope next to healthy ones, and nested inside them
    cc, w = R.words_of((200, [1.0, 0.0, 0.0]), (204, [2.0]), (204, [0.0]), _LEAF, (205, []), (205, []), (201, []), (0, [3.0, 0.0, 0.0, 0.5]), (100, []))
    assert decode(cc, w)["cull_veto"] == 1
    # a primitive that is not finite inside a healthy scope: its bounding sphere says nothing
    for leaf in ((0, [INF, 0.0, 0.0, 0.5]), (0, [0.0, 0.0, 0.0, INF]), (1, [0.0, 0.0, 0.0, 0.5, INF, 0.5]), (10, [0.0, math.nan, 0.0, 0.5, 0.5]),
                 (1, [0.0, 0.0, 0.0, 0.5, math.nan, 0.5]), (10, [0.0, 0.0, 0.0, math.nan, 0.5]), (10, [0.0, 0.0, 0.0, 0.5, math.nan])):
        assert decode(*_scoped((200, [1.0, 0.0, 0.0]), leaf))["cull_veto"] == 1, leaf
    # (a sphere of NaN radius has the value NaN everywhere, and every operator drops a NaN operand: it is not there at all)
    assert decode(*_scoped((200, [1.0, 0.0, 0.0]), (0, [0.0, 0.0, 0.0, math.nan])))["cull_veto"] == 0
    # a box or a cylinder with a NaN size is an infinite slab or column -- the NaN drops out of the leaf's maxima --, with or
    # without transforms: the tables and the walk on lower bounds would read max(NaN, 0) = 0, a flat leaf
    for leaf in ((1, [0.0, 0.0, 0.0, 0.5, math.nan, 0.5]), (10, [0.0, 0.0, 0.0, math.nan, 0.5]), (10, [0.0, 0.0, 0.0, 0.5, math.nan])):
        assert decode(*R.words_of(leaf, (0, [3.0, 0.0, 0.0, 0.5]), (100, [])))["cull_veto"] == 1, leaf
        q = np.array([[0.0, 50.0, 0.0], [50.0, 0.0, 0.0], [0.0, 0.0, 50.0]], dtype=F)
        with np.errstate(all="ignore"):
            v = onp.map_scene(*R.words_of(leaf), 100.0, q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy())
        assert v.min() <= 0.0, (leaf, v)            # (the binary32 oracle: the leaf reaches a point 50 away along some axis)
    # without transforms the tables are built from the parameters on the device, which vetoes there; the decoder only keeps the
    # lower-bound walk away from a scene it has no scale for
    d = decode(*R.words_of((0, [0.0, 0.0, 0.0, 1.0]), (0, [INF, 0.0, 0.0, 1.0]), (110, [0.25])))
    assert d["cull_veto"] == 0 and d["bound_walk"] == 0 and d["has_xforms"] == 0


def test_finite_programs_keep_their_culling(programs):
    """No named or generated program loses its culling to a veto: their transforms are similarities (the generators normalise
    their quaternions in binary64 and round them to binary32: squared norm within 1e-6 of 1)."""
    for name, cc, w, d in programs:
        assert d["cull_veto"] == 0, name
        blends = d["smooth_slack"] > 0.0
        sharper = any((r["kind"] == 4 and not r["nocull"]) or r["mode"] == 3 for r in d["rec"])
        assert d["bound_walk"] == int((blends or sharper) and not d["has_xforms"] and d["spill_depth"] <= 1), name


def test_subtracted_leaves_have_no_table_entry(programs):
    """RM_OP_NOCULL marks exactly the leaves inside the right operand of a Subtraction; without transforms the others' slots
    count up per table, with transforms every bounded leaf has a slot into `bounds`."""
    n_nocull = 0
    for name, cc, w, d in programs:
        cmds = [(op, a) for op, a, _ in R.commands(cc, w) if op != 300]
        # the right operand of every Subtraction, by walking the postfix program
        stack, sub = [], set()
        for i, (op, a) in enumerate(cmds):
            if op in (R.SPHERE, R.BOX, R.PLANE, R.CYLINDER):
                stack.append([i])
            elif op in (100, 101, 102, 110):
                b = stack.pop()
                a_ = stack.pop()
                if op == 101:
                    sub.update(b)
                stack.append(a_ + b)
        leaves = [r for r in d["rec"] if r["kind"] in (1, 2, 3, 4)]
        assert {r["cmd"] for r in leaves if r["nocull"]} == sub, name
        n_nocull += len(sub)
        if d["has_xforms"]:
            assert sorted(r["slot"] for r in leaves if r["kind"] != 4) == list(range(d["n_sphere"]))
        else:
            assert [r["slot"] for r in leaves if r["kind"] == 1 and not r["nocull"]] == list(range(d["n_sphere"])), name
            assert [r["slot"] for r in leaves if r["kind"] in (2, 3) and not r["nocull"]] == list(range(d["n_box"])), name
    assert n_nocull > 20
