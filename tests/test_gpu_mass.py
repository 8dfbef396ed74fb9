"""Mass properties on the GPU (rm_mass_moments): the sixteen moment words against the numpy restatement on
the oracle's lattice (tests/mass_ref.py: no bricks, no skipping) with ==, and the statistics against the brick-class model,
exactly; lattices on which bricks proven inside occur (the closed form); odd shapes; random programs; programs without a bound;
indices and sums beyond 32 bits; errors and isolation; mass_properties end to end."""
import ctypes as C

import numpy as np
import pytest

import fuzz_programs as FP
import mass_ref as M
import scenes
import sparse_ref
import test_mesh_bound_cpu as B
from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu

F = np.float32
ALL_SCENES = B.ALL_SCENES
MESH_SCENES = B.MESH_SCENES
LIM = (0.01, 100.0, 256)
STAT_KEYS = ("bricks", "bricks_kept", "bricks_inside", "evaluations")


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    r.set_materials(scenes.MATERIAL_TABLE)
    yield r
    r.close()


def cube(n, lo=-3.0, hi=3.0):
    return (lo,) * 3, (F(hi - lo) / F(n - 1),) * 3, (n, n, n)


def words_of(*cmds):
    out = []
    for op, params in cmds:
        out += [op] + [int(x) for x in np.asarray(params, dtype=F).view(np.uint32)]
    return len(cmds), np.asarray(out, dtype=np.uint32)


def sphere(r, centre=(0.0, 0.0, 0.0)):
    return words_of((0, list(centre) + [r]))


def use(res, cc, w, limits=LIM):
    res.set_limits(limits)
    res.set_program(cc, w)


def model_stats(cc, w, origin, step, shape, level, max_dist=LIM[1]):
    L, E = B.program_bound(cc, w, sparse_ref.lattice_P(origin, step, shape))
    keep, inside, stats = M.class_model(cc, w, origin, step, shape, level, L, E, max_dist)
    return keep, inside, stats, L, E


def check(res, cc, w, origin, step, shape, level=0.0, max_dist=LIM[1], want=None, what=""):
    """rm_mass_moments' sixteen words == the restatement's and its statistics == the class model's.  Returns (result, model stats)."""
    got = res.mass_moments(origin, step, shape, level)
    if want is None:
        want = M.lattice_moments(cc, w, origin, step, shape, level, max_dist)
    keep, inside, stats, L, E = model_stats(cc, w, origin, step, shape, level, max_dist)
    print("%s %s level %g: L = %.6g E = %.3g; stats %s (model %s); moments %s" % (what, shape, level, L, E, got.stats, stats,
                                                                                 [int(x) for x in got.moments]))
    assert got.moments.dtype == np.uint64 and got.moments.shape == (16,)
    assert [int(x) for x in got.moments] == want, (what, shape, level)
    assert {k: got.stats[k] for k in STAT_KEYS} == stats, (what, shape, level)
    # memory: 4 B per brick and per 256 bricks a block sum (8 B) and a row (128 B); per kept brick its index and its row; the
    # totals, the result row and the regions' rounding to 16 bytes in the last term
    assert 0 < got.stats["scratch_bytes"] <= 4 * (stats["bricks"] + 1) + 136 * (stats["bricks"] // 256 + 1) + 132 * stats["bricks_kept"] + 256
    return got, stats


# ---- equality with the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESH_SCENES)
def test_named_scenes(res, oracle, name):
    cc, w = oracle.serialize(*ALL_SCENES[name]())
    use(res, cc, w)
    origin, step, shape = cube(72)
    for level in (0.0, 0.05):
        got, stats = check(res, cc, w, origin, step, shape, level, what=name)
        assert got.moments[0] > 0 and stats["bricks_kept"] < stats["bricks"]


ODD = (((-0.2, 0.1, -0.3), (0.6, 0.5, 0.7), (2, 2, 2)),
       ((-1.0, -2.1, -0.2), (0.9, 0.55, 0.7), (3, 9, 2)),
       ((-3.0, -0.35, -2.0), (0.1, 0.12, 0.031), (61, 7, 130)),
       ((-3.0, -2.5, -2.0), (0.15, 0.14, 0.15), (33, 41, 25)),
       ((0.3, -7.0, 1e-3), (0.01, 0.4, 0.123), (41, 37, 29)))


@pytest.mark.parametrize("name", ["g32", "xform_mix"])
def test_odd_shapes(res, oracle, name):
    cc, w = oracle.serialize(*ALL_SCENES[name]())
    use(res, cc, w)
    for origin, step, shape in ODD:
        check(res, cc, w, origin, step, shape, what=name)


@pytest.mark.parametrize("cls,seed", [(cls, seed) for cls in FP.CLASSES for seed in range(4)])
def test_random_programs(res, oracle, cls, seed):
    c = FP.case(oracle, cls, seed)
    res.set_materials(c.table)
    try:
        use(res, c.cc, c.words, c.limits)
        origin, step, shape = cube(40)
        level = (0.0, 0.03, -0.02)[seed % 3]
        check(res, c.cc, c.words, origin, step, shape, level, max_dist=c.limits[1], what=FP.describe(c))
    finally:
        res.set_materials(scenes.MATERIAL_TABLE)


# ---- bricks proven inside ---------------------------------------------------------------------------------------------------------
def test_inside_bricks_on_a_sphere(res):
    cc, w = sphere(2.5)
    use(res, cc, w)
    for (origin, step, shape), want in ((cube(72), (317, 90, 322)),
                                        (((-3.0, -2.5, -2.0), (0.09, 0.11, 0.1), (61, 47, 39)), (159, 52, 29))):
        got, stats = check(res, cc, w, origin, step, shape, what="sphere 2.5")
        s = got.stats
        assert s["bricks_inside"] > 0
        assert (s["bricks_kept"], s["bricks_inside"], s["bricks"] - s["bricks_kept"] - s["bricks_inside"]) == want


@pytest.mark.parametrize("label, want", [("72 step 0.0125", (285, 34)), ("72 step 2^-7", (415, 200)), ("96 step 2^-8", (1728, 0))])
def test_far_lattices(res, label, want):
    """Coordinates of magnitude 800: E decides bricks; at step 2^-8 2 E > L r / 2 and every brick is kept."""
    cc, w = B.far_program()
    origin, step, shape = B.far_lattices()[label]
    use(res, cc, w)
    got, stats = check(res, cc, w, origin, step, shape, what="far " + label)
    assert (got.stats["bricks_kept"], got.stats["bricks_inside"]) == want
    assert got.moments[0] > 0
    if want[1]:
        assert got.stats["bricks_inside"] > 0
    else:
        assert got.stats["bricks_kept"] == got.stats["bricks"] == 1728


# ---- programs without a bound -----------------------------------------------------------------------------------------------------
def unbounded_programs():
    sph, box = (0, [0.2, 0.1, -0.1, 0.9]), (1, [-0.4, 0.0, 0.3, 0.5, 0.6, 0.4])
    return {"scale 0": words_of(sph, (204, [0.0]), box, (205, []), (100, [])),
            "non-finite parameter": words_of(sph, (1, [-0.4, np.inf, 0.3, 0.5, 0.6, 0.4]), (100, []))}


@pytest.mark.parametrize("label", sorted(unbounded_programs()))
def test_programs_without_a_bound_keep_every_brick(res, label):
    cc, w = unbounded_programs()[label]
    use(res, cc, w)
    assert np.isinf(renderer.program_lipschitz(cc, w))
    origin, step, shape = cube(40, -2.0, 2.0)
    got, stats = check(res, cc, w, origin, step, shape, what=label)
    assert got.stats["bricks_kept"] == got.stats["bricks"] == 125 and got.stats["bricks_inside"] == 0
    assert got.stats["evaluations"] == 125 + 40 ** 3


def test_the_empty_program(res):
    cc, w = 0, np.zeros(0, dtype=np.uint32)
    use(res, cc, w)
    origin, step, shape = cube(37, -2.0, 2.0)
    got, stats = check(res, cc, w, origin, step, shape, 0.0, what="empty")
    assert [int(x) for x in got.moments] == [0] * 10 + [0xFFFFFFFF] * 3 + [0] * 3
    # level above max_dist: every point is inside.  The program's bound is L = 0 and E = 0, so section 15's rule as it stands
    # (margin 0, and 2 E <= L r / 2 holds as 0 <= 0) clears every brick and the probe (max_dist < level) classes it inside: the
    # statistics are the model's (check), and all of N comes from the closed form
    got, stats = check(res, cc, w, origin, step, shape, 1000.0, want=M.box_moments((0, 0, 0), shape), what="empty")
    assert int(got.moments[0]) == 37 ** 3 and got.stats["bricks"] == 125


# ---- beyond 32 bits ---------------------------------------------------------------------------------------------------------------
BIG = (4096, 4096, 256)


def big_lattice():
    lo, step, n = renderer.RayMarchingResources._box_lattice(-1.0, 1.0, BIG)
    return tuple(lo), tuple(step), BIG


def test_every_brick_inside_on_2_to_the_32_points(res):
    """Sphere r = 8 about a lattice in [-1, 1]^3: no brick is kept, all 2^23 are inside, N = 2^32 and sum i^2 is about 2^55: a
    32-bit count or any floating accumulation cannot give these words."""
    cc, w = sphere(8.0)
    use(res, cc, w)
    origin, step, shape = big_lattice()
    keep, inside, stats, L, E = model_stats(cc, w, origin, step, shape, 0.0)
    print("L = %g, E = %.3g, model %s" % (L, E, stats))
    assert stats["bricks"] == 2 ** 23 and stats["bricks_kept"] == 0 and stats["bricks_inside"] == 2 ** 23
    got = res.mass_moments(origin, step, shape, 0.0)
    want = M.box_moments((0, 0, 0), shape)
    print(got.stats, [int(x) for x in got.moments])
    assert want[0] == 2 ** 32 and want[4] > 2 ** 54
    assert [int(x) for x in got.moments] == want
    assert {k: got.stats[k] for k in STAT_KEYS} == stats and got.stats["evaluations"] == 2 ** 23


def test_a_small_solid_at_the_far_corner_of_a_large_lattice(res):
    """Sphere r = 0.05 at (1, 1, 1): the kept bricks lie at brick coordinates near (511, 511, 31), where i0^2 c exceeds 2^32 in the
    shift to lattice coordinates.  The reference is the restatement on the index box i, j >= 3936, k >= 248 (offset indices); the
    model shows that no kept or inside brick lies outside it."""
    cc, w = sphere(0.05, (1.0, 1.0, 1.0))
    use(res, cc, w)
    origin, step, shape = big_lattice()
    keep, inside, stats, L, E = model_stats(cc, w, origin, step, shape, 0.0)
    print("L = %g, E = %.3g, model %s" % (L, E, stats))
    first = (3936, 3936, 248)
    kz, ky, kx = np.nonzero(keep | inside)
    assert len(kz) > 0 and kx.min() >= first[0] // 8 and ky.min() >= first[1] // 8 and kz.min() >= first[2] // 8
    assert stats["bricks_kept"] == 279 and stats["bricks_inside"] == 0
    want = M.moments_of_inside(M.lattice_inside(cc, w, origin, step, shape, 0.0, LIM[1], first=first), first)
    got = res.mass_moments(origin, step, shape, 0.0)
    print(got.stats, [int(x) for x in got.moments])
    assert want[0] > 0 and want[4] > 2 ** 32
    assert [int(x) for x in got.moments] == want
    assert {k: got.stats[k] for k in STAT_KEYS} == stats


# ---- agreement with the mesh, determinism, isolation --------------------------------------------------------------------------------
def test_kept_bricks_are_the_sparse_mesh_s_and_two_runs_agree(res, oracle):
    cc, w = oracle.serialize(*scenes.g32())
    use(res, cc, w)
    for origin, step, shape in (cube(72), ODD[2], ODD[4]):
        for level in (0.0, 0.05):
            a = res.mass_moments(origin, step, shape, level)
            b = res.mass_moments(origin, step, shape, level)
            assert a.moments.tobytes() == b.moments.tobytes() and a.stats == b.stats
            m = res.extract_mesh_grid_sparse(origin, step, shape, level=level, normals=False, ids=False)
            assert a.stats["bricks_kept"] == m.stats["bricks_kept"] and a.stats["bricks"] == m.stats["bricks"]


def test_draws_and_the_context_mesh_are_left_alone(res, oracle):
    cc, w = oracle.serialize(*scenes.xform_mix())
    W, H = 64, 48
    res.set_limits((0.01, 100.0, 128))
    res.set_program(cc, w)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    first = res.draw(W, H)
    origin, step, shape = cube(40)
    mesh = res.extract_mesh_grid_sparse(origin, step, shape)
    assert len(mesh.triangles) > 0
    got = res.mass_moments(*cube(56))
    assert got.moments[0] > 0
    assert res.draw(W, H).tobytes() == first.tobytes()
    v, t = np.empty((len(mesh.vertices), 3), dtype=np.float32), np.empty((len(mesh.triangles), 3), dtype=np.uint32)
    res._check(res._L.rm_read_mesh(res._h, v.ctypes.data, t.ctypes.data, None, None, 0, None))
    assert v.tobytes() == mesh.vertices.tobytes() and t.tobytes() == mesh.triangles.tobytes()


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def lattice(o=(0.0, 0.0, 0.0), s=(0.1, 0.1, 0.1)):
    return (C.c_float * 3)(*o), (C.c_float * 3)(*s)


def test_errors(res, oracle):
    L = _ffi.hip_lib()
    cc, w = oracle.serialize(*scenes.g8())
    use(res, cc, w)
    o, s = lattice()
    NM, NS = _ffi.RM_MOMENTS, _ffi.RM_MASS_STATS
    mom, stats = (C.c_uint64 * NM)(), (C.c_uint64 * NS)()
    call = lambda h=res._h, o=o, s=s, n=(4, 4, 4), level=0.0, mom=mom, nm=NM, stats=stats, ns=NS: \
        L.rm_mass_moments(h, o, s, n[0], n[1], n[2], level, mom, nm, stats, ns)   # noqa: E731
    assert call() == _ffi.RM_OK
    assert call(h=None) == _ffi.RM_ERR_NULL
    assert call(mom=None) == _ffi.RM_ERR_NULL
    assert call(stats=None) == _ffi.RM_ERR_NULL
    assert call(o=None) == _ffi.RM_ERR_NULL and call(s=None) == _ffi.RM_ERR_NULL
    assert call(nm=NM - 1) == _ffi.RM_ERR_ARG
    assert call(ns=NS - 1) == _ffi.RM_ERR_ARG
    for n in ((1, 4, 4), (4, 4, 1), (4097, 2, 2), (2, 65536, 2)):
        assert call(n=n) == _ffi.RM_ERR_RANGE, n
    assert call(n=(2, 2, 2)) == _ffi.RM_OK
    for bad in ((0.1, 0.0, 0.1), (0.1, -0.1, 0.1), (np.inf, 0.1, 0.1), (np.nan, 0.1, 0.1)):
        assert call(s=lattice(s=bad)[1]) == _ffi.RM_ERR_ARG, bad
    assert call(o=lattice(o=(0.0, np.inf, 0.0))[0]) == _ffi.RM_ERR_ARG
    for level in (np.nan, np.inf):
        assert call(level=level) == _ffi.RM_ERR_ARG
    with pytest.raises(ValueError):
        res.mass_moments((0, 0, 0), (0.1, 0.1, 0.1), (1, 4, 4))
    # an invalid program: the status a query gives
    res.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([1, 100], np.uint32).tobytes())   # Union on an empty stack
    assert call() == _ffi.RM_ERR_STACK_UNDERFLOW


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_mass_properties_of_g32(res, oracle):
    cc, w = oracle.serialize(*scenes.g32())
    use(res, cc, w)
    lo, hi, n, density = (-2.5,) * 3, (2.5,) * 3, 72, 2.7
    p = res.mass_properties(lo, hi, n, density=density)
    origin, step, shape = cube(n, -2.5, 2.5)
    m = M.lattice_moments(cc, w, origin, step, shape, 0.0)
    assert [int(x) for x in p["moments"]] == m
    want = M.from_moments(m, origin, step, density)
    tol = M.tolerances(want, origin, step, shape)
    got = [p["volume"], p["mass"]] + list(p["centroid"]) + [p["inertia"][0, 0], p["inertia"][1, 1], p["inertia"][2, 2], p["inertia"][0, 1],
                                                            p["inertia"][1, 2], p["inertia"][0, 2]] + list(p["bbox_lo"]) + list(p["bbox_hi"])
    print(p)
    for e in range(_ffi.RM_MASS_PROPS):
        assert abs(got[e] - want[e]) <= tol[e], (e, got[e], want[e])
    assert p["volume"] > 1.0 and np.array_equal(p["inertia"], p["inertia"].T)
    assert np.all(p["bbox_lo"] < p["centroid"]) and np.all(p["centroid"] < p["bbox_hi"])
