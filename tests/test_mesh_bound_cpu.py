"""What sparse mesh extraction takes on trust, without a GPU: rm_program_bound's evaluation error E against
a binary64 evaluation of the scene (tests/scene_f64.py), how E and L behave in P, and a numpy model of the brick skipping rule
(tests/sparse_ref.py) that must never clear a brick whose tile the surface crosses -- on the named scenes and on lattices far
from the origin with steps down to the coordinates' ulp, where E decides.  tests/cpp/bound_probe.cpp makes E readable: the C ABI
returns only L."""
import atexit
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import mesh_ref
import scene_f64
import scenes
import sparse_ref
import test_gpu_fuzz
import test_sparse_mesh_cpu as T
from oracle import rm_oracle_np as onp
from ray_marching_amd import _ffi, renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ALL_SCENES = T.ALL_SCENES
MESH_SCENES = ("g1", "g8", "g32", "g32_balanced", "g8x", "g32s", "ext_mix", "xform_mix", "mat_mix")
MAX_DIST = 100.0


# ---- E and L from rm_program_bound ---------------------------------------------------------------------------------------------
_PROBE = []


def _probe_exe():
    if not _PROBE:
        d = tempfile.mkdtemp(prefix="rm_bound_probe_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "bound_probe")
        b = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "cpp", "bound_probe.cpp")], capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr[-3000:]
        _PROBE.append(exe)
    return _PROBE[0]


def program_bounds(cc, words, Ps):
    """[(status, L, E)] of rm_program_bound at every P of Ps."""
    w = [int(x) for x in np.asarray(words, dtype=np.uint32)]
    text = "%d %d\n%s\n%s\n" % (cc, len(w), " ".join(map(str, w)), " ".join("%.17g" % float(P) for P in Ps))
    run = subprocess.run([_probe_exe()], input=text, capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.returncode, run.stderr[-1000:])
    rows = [line.split() for line in run.stdout.splitlines()]
    assert len(rows) == len(Ps), run.stdout[-1000:]
    return [(int(r[0]), float(r[1]), float(r[2])) for r in rows]


def program_bound(cc, words, P):
    """(L, E) of rm_program_bound for points with |coordinates| <= P; the program must decode."""
    (status, L, E), = program_bounds(cc, words, [P])
    assert status == 0, "rm_program_bound: status %d" % status
    return L, E


# ---- the lattices far from the origin (shared with the GPU tests) -------------------------------------------------------------
FAR_CENTRE = (800.0, -300.0, 500.0)


def far_program():
    """Sphere r = 0.3 at (800, -300, 500) united with a box and a cylinder next to it: no transform, so every leaf subtracts
    coordinates of magnitude 800 and E is about 9e-3."""
    x, y, z = FAR_CENTRE
    return T.words_of((0, [x, y, z, 0.3]), (1, [x + 0.25, y - 0.2, z + 0.1, 0.12, 0.08, 0.1]), (100, []),
                      (10, [x - 0.15, y + 0.1, z + 0.2, 0.1, 0.15]), (100, []))


def centred(centre, step, n):
    return tuple(float(F(c - 0.5 * (n - 1) * step)) for c in centre), (F(step),) * 3, (n, n, n)


def far_lattices():
    """label -> (origin, step, shape).  With L = 1 and E = 9.2e-3: at steps 0.0125 and 2^-7 the error term is a fifth to a third of
    L r (it decides bricks); at 2^-8 it exceeds L r / 4 and every brick is kept."""
    c = (FAR_CENTRE[0] + 0.1, FAR_CENTRE[1] - 0.05, FAR_CENTRE[2] + 0.05)
    return {"72 step 0.0125": centred(c, 0.0125, 72), "72 step 2^-7": centred(c, 2.0 ** -7, 72), "96 step 2^-8": centred(c, 2.0 ** -8, 96)}


def near_ulp_lattice():
    """72^3 with step 2^-15 about a point of the far sphere's surface: half an ulp of x = 800 (about every second x coordinate
    repeats the one before), one ulp of y and z."""
    h = 0.3 / math.sqrt(3.0)
    return centred((FAR_CENTRE[0] + h, FAR_CENTRE[1] + h, FAR_CENTRE[2] + h), 2.0 ** -15, 72)


def oracle_grid(cc, w, origin, step, shape):
    p = mesh_ref.lattice_points(origin, step, shape)
    with np.errstate(all="ignore"):
        d = onp.map_scene(cc, w, F(MAX_DIST), p[:, 0], p[:, 1], p[:, 2])
    return np.asarray(d, dtype=F).reshape(shape[2], shape[1], shape[0])


# ---- the binary64 reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL_SCENES))
def test_scene_f64_agrees_with_the_binary32_oracle(oracle, name):
    cc, w = oracle.serialize(*ALL_SCENES[name]())
    p = np.random.default_rng(64).uniform(-4.0, 4.0, (10000, 3)).astype(F)
    d32 = onp.map_scene(cc, w, F(MAX_DIST), p[:, 0], p[:, 1], p[:, 2]).astype(np.float64)
    d64 = scene_f64.map_scene(cc, w, MAX_DIST, p)
    assert d64.dtype == np.float64 and d64.shape == (10000,)
    assert np.all(np.abs(d32 - d64) <= 1e-4 + 1e-6 * np.abs(d64)), float(np.abs(d32 - d64).max())
    assert np.abs(d32 - d64).max() > 0.0          # ... and it is not the binary32 value widened


def test_scene_f64_known_answers():
    p = np.array([[3.0, 4.0, 12.0], [0.25, -0.5, 0.125]])
    f = lambda *cmds: scene_f64.map_scene(*T.words_of(*cmds), MAX_DIST, p)
    assert np.array_equal(f((0, [0, 0, 0, 1.0])), [12.0, math.sqrt(0.328125) - 1.0])
    assert np.array_equal(f((1, [0, 0, 0, 1.0, 1.0, 2.0])), [math.sqrt(4.0 + 9.0 + 100.0), -0.5])
    assert np.array_equal(f((2, [0.0, 2.0, 0.0, 0.5])), [8.5, -0.5])
    assert np.array_equal(f((10, [0, 0, 0, 5.0, 1.0])), [math.hypot(math.hypot(3.0, 12.0) - 5.0, 3.0), -0.5])
    s, b = (0, [0, 0, 0, 1.0]), (2, [0.0, 2.0, 0.0, 0.5])
    assert np.array_equal(f(s, b, (100, [])), [8.5, -0.5])
    assert np.array_equal(f(s, b, (101, [])), [12.0, 0.5])
    assert np.array_equal(f(s, b, (102, [])), [12.0, math.sqrt(0.328125) - 1.0])
    assert np.array_equal(f(s, b, (110, [-1.0])), [8.5, -0.5])
    a, c = math.sqrt(0.328125) - 1.0, -0.5
    assert np.allclose(f(s, b, (110, [0.5])), [8.5, min(a, c) - (0.5 - abs(a - c)) ** 2 / (4 * 0.5)], rtol=1e-15, atol=0)
    assert np.array_equal(f((200, [1.0, 1.0, 0.0]), b, (201, [])), [6.5, -2.5])
    assert np.array_equal(f((204, [0.5]), s, (205, [])), [12.5, math.sqrt(0.328125) - 0.5])
    h = math.sqrt(0.5)       # a quarter turn about z: for (w, a) = (h, 0, 0, h) the position formula takes (x, y, z) to (y, -x, z)
    got = f((202, [h, 0.0, 0.0, h]), (2, [1.0, 0.0, 0.0, 0.0]), (203, []))
    hf = float(F(h))
    assert np.allclose(got, [(1 - 2 * hf * hf) * 3.0 + 2 * hf * hf * 4.0, (1 - 2 * hf * hf) * 0.25 - 2 * hf * hf * 0.5], rtol=1e-14, atol=1e-15)
    assert np.allclose(got, [4.0, -0.5], rtol=0, atol=1e-6)
    assert np.array_equal(scene_f64.map_scene(0, [], 7.0, p), [7.0, 7.0])


# ---- the programs ----------------------------------------------------------------------------------------------------------------
def random_programs(oracle, count=40, first_seed=31000):
    """`count` valid random programs (depth 2-4, planes in every second one), and for those with planes or rotations the same tree
    with scaled plane normals and off-unit quaternions."""
    out, seed = [], first_seed
    while sum(1 for label, *_ in out if "scaled" not in label) < count:
        rng = np.random.default_rng(seed)
        t = scenes._Tab()
        root = test_gpu_fuzz.random_tree(rng, t, int(rng.integers(2, 5)), allow_plane=seed % 2 == 0, tags=bool(rng.random() < 0.3))
        cc, w = oracle.serialize(t.nodes, root)
        if oracle.validate(cc, w)[0] == 0:
            out.append(("seed %d" % seed, cc, w))
            if any(k in (scenes.PLANE, scenes.ROTATION) for k, *_ in t.nodes):
                out.append(("seed %d, scaled planes and quaternions" % seed, *oracle.serialize(T.variants(rng, t.nodes), root)))
        seed += 1
    return out


def stress_programs(oracle):
    def one(label, build):
        t = scenes._Tab()
        return (label, *oracle.serialize(t.nodes, build(t)))
    ball = lambda t: t.sphere((0.3, -0.2, 0.1), 0.5)
    pair = lambda t: (t.sphere((0.4, 0.1, -0.3), 0.6), t.box((-0.3, 0.2, 0.2), (0.5, 0.3, 0.4)))

    def four_rotations(t):
        node = t.op(scenes.UNION, t.box((0.2, -0.1, 0.3), (0.6, 0.3, 0.4)), t.cylinder((-0.5, 0.2, 0.0), 0.3, 0.6))
        for ang, ax in ((0.7, (1, 2, -1)), (-2.1, (0, 1, 1)), (1.3, (3, -1, 2)), (2.9, (-1, -1, 4))):
            a = np.asarray(ax, dtype=np.float64) / np.linalg.norm(ax)
            node = t.rotation(node, (math.cos(ang / 2), *(math.sin(ang / 2) * a)))
        return node
    return [one("scale 1e-3 around a sphere", lambda t: t.scale(ball(t), 1e-3)),
            one("scale 50 around a sphere", lambda t: t.scale(ball(t), 50.0)),
            one("four nested rotations", four_rotations),
            one("translation by (800, -300, 500)", lambda t: t.translation(t.op(scenes.UNION, *pair(t)), (800.0, -300.0, 500.0))),
            one("smooth union k = 0.02", lambda t: t.smooth_union(*pair(t), 0.02)),
            one("smooth union k = 5", lambda t: t.smooth_union(*pair(t), 5.0))]


# ---- E ---------------------------------------------------------------------------------------------------------------------------
N_POINTS = 50000


def test_evaluation_error_bound_is_sound(oracle):
    """|oracle_np(p) - scene_f64(p)| <= E(P) at every one of 50 000 binary32 points of [-P, P]^3, for P = 3 and P = 1000: the claim
    of DESIGN.md section 15 "The evaluation error" (the oracle's values are the kernels', bit for bit: tests/test_gpu_mesh.py)."""
    progs = random_programs(oracle) + stress_programs(oracle)
    worst_ratio, worst_label, E_lo, E_hi = 0.0, None, math.inf, 0.0
    for P in (3.0, 1000.0):
        pts = np.random.default_rng(int(P)).uniform(-P, P, (N_POINTS, 3)).astype(F)
        pts = np.clip(pts, F(-P), F(P))
        counted = 0
        for label, cc, w in progs:
            L, E = program_bound(cc, w, P)
            if math.isinf(E):
                continue
            counted += 1
            with np.errstate(all="ignore"):
                d32 = onp.map_scene(cc, w, F(MAX_DIST), pts[:, 0], pts[:, 1], pts[:, 2]).astype(np.float64)
            err = np.abs(d32 - scene_f64.map_scene(cc, w, MAX_DIST, pts))
            assert np.all(np.isfinite(err)), (label, P)
            ratio = float(err.max() / E)
            if ratio > worst_ratio:
                worst_ratio, worst_label = ratio, "%s at P = %g" % (label, P)
            E_lo, E_hi = min(E_lo, E), max(E_hi, E)
            assert np.all(err <= E), (label, P, float(err.max()), E)
        assert counted >= 40, (P, counted)
    print("largest |oracle - f64| / E: %.4f (%s); E from %.3g to %.3g over %d programs" % (worst_ratio, worst_label, E_lo, E_hi, len(progs)))


def test_bound_grows_with_P_and_rejects_what_it_cannot_cover(oracle):
    Ps = [1.0, 3.0, 10.0, 100.0, 1000.0, 1.0e4, 1.0e6]
    for label, cc, w in random_programs(oracle) + stress_programs(oracle):
        rows = program_bounds(cc, w, Ps)
        assert all(status == 0 for status, _, _ in rows), label
        E = [e for _, _, e in rows]
        assert all(e > 0.0 for e in E) and all(a <= b for a, b in zip(E, E[1:])), (label, E)
        assert all(math.isinf(l) == math.isinf(e) for _, l, e in rows), label
        assert rows[0][1] == renderer.program_lipschitz(cc, w), label          # rm_program_lipschitz evaluates at P = 1
        finite = [l for _, l, _ in rows if math.isfinite(l)]
        assert len(set(finite)) <= 1, (label, finite)                          # L does not depend on P
    # the cases test_lipschitz_fixed_cases lists: +inf for exactly those it lists as infinite
    sphere = (0, [0.1, 0.2, 0.3, 0.5])
    infinite = [T.words_of((204, [0.0]), sphere, (205, [])), T.words_of((0, [0.1, np.nan, 0.3, 0.5])),
                T.words_of(sphere, sphere, (110, [np.inf]))]
    finite = [T.words_of(sphere), T.words_of((0, [0, 0, 0, -0.3])), T.words_of((1, [0, 0, 0, 0.0, -1.0, 0.5])),
              T.words_of((204, [-0.7]), sphere, (205, [])), T.words_of((204, [1e-3]), sphere, (205, [])),
              T.words_of((202, [2.0, 0.0, 0.0, 0.0]), sphere, (203, [])), T.words_of((2, [0.0, 1.0, 0.2, 0.5])),
              T.words_of(sphere, (2, [3.0, 0.0, 4.0, 0.5]), (110, [0.3]))]
    finite += [T.words_of((202, list(q)), sphere, (203, [])) for q in ((1.3, 0.2, -0.4, 0.5), (0.5, 0.5, 0.5, 0.5), (0.3, 0.9, 0.1, -0.2))]
    for cc, w in infinite:
        for P in (1.0, 1000.0):
            L, E = program_bound(cc, w, P)
            assert math.isinf(L) and math.isinf(E) and L > 0 and E > 0, (list(w), P)
        assert math.isinf(renderer.program_lipschitz(cc, w))
    for cc, w in finite:
        for P in (1.0, 1000.0):
            L, E = program_bound(cc, w, P)
            assert math.isfinite(L) and math.isfinite(E) and E > 0.0, (list(w), P)
        assert program_bound(cc, w, 1.0)[0] == renderer.program_lipschitz(cc, w)
    assert program_bound(0, [], 5.0) == (0.0, 0.0)                             # the empty program: a constant
    assert program_bounds(1, [100], [1.0])[0][0] == _ffi.RM_ERR_STACK_UNDERFLOW
    L, E = program_bound(*T.words_of(sphere), math.inf)                        # no finite P: nothing is proven
    assert math.isinf(L) and math.isinf(E)


# ---- the skipping rule -----------------------------------------------------------------------------------------------------------
def model_counts(cc, w, origin, step, shape, level, dist):
    """(keep flags, keep flags with E = 0, mixed flags) of one lattice; asserts that no mixed brick is cleared."""
    L, E = program_bound(cc, w, sparse_ref.lattice_P(origin, step, shape))
    keep, evals = sparse_ref.brick_model(cc, w, origin, step, shape, level, L, E)
    keep0, _ = sparse_ref.brick_model(cc, w, origin, step, shape, level, L, 0.0)
    mixed = sparse_ref.mixed_bricks(dist, level)
    assert keep.shape == mixed.shape and evals >= keep.size
    assert not np.any(mixed & ~keep), "the rule clears %d bricks whose tile the surface crosses" % int(np.count_nonzero(mixed & ~keep))
    return keep, keep0, mixed, E


def test_brick_model_never_clears_a_mixed_brick(oracle):
    for name in MESH_SCENES:
        cc, w = oracle.serialize(*ALL_SCENES[name]())
        origin, step, shape = (-3.0,) * 3, (F(6.0) / F(71),) * 3, (72,) * 3
        dist = oracle_grid(cc, w, origin, step, shape)
        for level in (0.0, 0.05):
            keep, keep0, mixed, E = model_counts(cc, w, origin, step, shape, level, dist)
            assert 0 < np.count_nonzero(mixed) <= np.count_nonzero(keep) < keep.size, (name, level)
    cc, w = far_program()
    rows = {}
    for label, (origin, step, shape) in far_lattices().items():
        dist = oracle_grid(cc, w, origin, step, shape)
        for level in (0.0, 0.03):
            keep, keep0, mixed, E = model_counts(cc, w, origin, step, shape, level, dist)
            assert not np.any(mixed & ~keep0)          # E = 0 still holds on the oracle here: the bound is not the binding term
            if level == 0.0:
                rows[label] = (int(np.count_nonzero(keep)), int(np.count_nonzero(keep0)), int(np.count_nonzero(mixed)), keep.size)
                print("far lattice %s: E = %.3g, kept %d, kept with E = 0 %d, mixed %d of %d bricks" % ((label, E) + rows[label]))
    # the regimes the far lattices exist for really occur: E decides bricks at the first two, and keeps all at the third
    for label in ("72 step 0.0125", "72 step 2^-7"):
        kept, kept0, mixed, bricks = rows[label]
        assert bricks > kept > kept0 > mixed > 0, (label, rows[label])
    kept, kept0, mixed, bricks = rows["96 step 2^-8"]
    assert kept == bricks > kept0 > mixed > 0, rows["96 step 2^-8"]
    origin, step, shape = near_ulp_lattice()
    dist = oracle_grid(cc, w, origin, step, shape)
    keep, keep0, mixed, E = model_counts(cc, w, origin, step, shape, 0.0, dist)
    xs = mesh_ref.axis_coords(origin, step, shape)[0]
    assert 30 <= len(np.unique(xs)) <= 42 and np.all(np.diff(xs) >= 0)          # about half of the 72 x coordinates are distinct
    assert keep.all() and np.count_nonzero(mixed) > 0
