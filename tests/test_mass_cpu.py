"""Mass properties without a GPU: the enums of the three faces (C header, ctypes, Rust), rm_mass_from_moments
against exact rational arithmetic (tests/mass_ref.py), the brick-class model (a cleared brick's own points are never mixed, an
inside brick's are all inside), and the quadrature's error bound on a sphere."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import mass_ref as M
import sparse_ref
import test_mesh_bound_cpu as B
import test_sparse_mesh_cpu as T
from ray_marching_amd import _ffi, renderer

F = np.float32
MESH_SCENES = B.MESH_SCENES
MAX_DIST = 100.0


# ---- the C, Rust and Python faces ----------------------------------------------------------------------------------------------
MOMENT_NAMES = ("COUNT", "X", "Y", "Z", "XX", "YY", "ZZ", "XY", "YZ", "XZ", "MIN_X", "MIN_Y", "MIN_Z", "MAX_X", "MAX_Y", "MAX_Z")
STAT_NAMES = ("BRICKS", "BRICKS_KEPT", "BRICKS_INSIDE", "EVALUATIONS", "SCRATCH_BYTES")
PROP_NAMES = ("VOLUME", "MASS", "CX", "CY", "CZ", "IXX", "IYY", "IZZ", "IXY", "IYZ", "IXZ", "LO_X", "LO_Y", "LO_Z", "HI_X", "HI_Y", "HI_Z")
ENUMS = {"rm_moment": dict([("RM_MOMENT_" + n, i) for i, n in enumerate(MOMENT_NAMES)] + [("RM_MOMENTS", 16)]),
         "rm_massstat": dict([("RM_MASS_STAT_" + n, i) for i, n in enumerate(STAT_NAMES)] + [("RM_MASS_STATS", 5)]),
         "rm_massprop": dict([("RM_MASS_" + n, i) for i, n in enumerate(PROP_NAMES)] + [("RM_MASS_PROPS", 17)])}


def test_symbols_and_constants():
    text, rust, L = T.header_text(), T.rust_text(), _ffi.hip_lib()
    for name in ("rm_mass_moments", "rm_mass_from_moments"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert hasattr(L, name), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    for tag, want in ENUMS.items():
        body = re.search(r"enum\s+%s\s*\{(.*?)\}" % tag, text, re.S).group(1)
        assert {n: int(v) for n, v in re.findall(r"(RM_[A-Z0-9_]+)\s*=\s*(-?\d+)", body)} == want, tag
        for name, value in want.items():
            assert getattr(_ffi, name) == value, name
            assert re.search(r"pub const %s: c_int = %d;" % (name, value), rust), name
    assert len(_ffi.MASS_STAT_NAMES) == _ffi.RM_MASS_STATS and len(renderer.MASS_PROP_NAMES) == _ffi.RM_MASS_PROPS
    assert re.search(r"#define RM_ABI_VERSION 2\b", text) and L.rm_abi_version() == 2
    o, s = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    mom, stats = (C.c_uint64 * 16)(), (C.c_uint64 * 5)()
    assert L.rm_mass_moments(None, o, s, 4, 4, 4, 0.0, mom, 16, stats, 5) == _ffi.RM_ERR_NULL


def test_rust_wrappers_check_their_slices_before_the_call():
    rust = T.rust_text()
    body = rust[rust.index("pub fn mass_moments("):]
    body = body[:body.index("\n    }\n")]
    assert body.index("assert!(out_moments.len() >= RM_MOMENTS as usize") < body.index("rm_mass_moments(")
    assert body.index("assert!(out_stats.len() >= RM_MASS_STATS as usize") < body.index("rm_mass_moments(")
    body = rust[rust.index("pub fn mass_from_moments("):]
    body = body[:body.index("\n}\n")]
    assert body.index("assert!(moments.len() >= RM_MOMENTS as usize") < body.index("rm_mass_from_moments(")
    assert body.index("assert!(out.len() >= RM_MASS_PROPS as usize") < body.index("rm_mass_from_moments(")


def test_cli_parses(capsys):
    from ray_marching_amd import massprops
    with pytest.raises(SystemExit):
        massprops.main(["--help"])
    out = capsys.readouterr().out
    assert "--density" in out and "--program" in out and "--level" in out


def test_cli_report_is_plain_json(tmp_path):
    import json
    from ray_marching_amd import massprops
    m = np.array(M.box_moments((1, 2, 3), (9, 8, 7)), dtype=np.uint64)
    props = renderer.mass_from_moments(m, (0.0, 0.0, 0.0), (0.5, 0.5, 0.5), 2.0)
    props["moments"], props["stats"] = m, {"bricks": 8, "bricks_kept": 0, "bricks_inside": 1, "evaluations": 8, "scratch_bytes": 64}
    r = json.loads(json.dumps(massprops.report(props)))
    assert sorted(r) == ["moments", "properties", "stats"] and r["moments"] == [int(x) for x in m]
    assert r["properties"]["volume"] == 8 * 6 * 4 * 0.125 and len(r["properties"]["inertia"]) == 3
    f = tmp_path / "p.json"
    f.write_text(json.dumps({"cmd_count": 1, "words": [0, 0, 0, 0, 0x3F800000]}))
    assert massprops.load_program(str(f)) == (1, [0, 0, 0, 0, 0x3F800000])


# ---- rm_mass_from_moments ---------------------------------------------------------------------------------------------------------
def check_from_moments(m, origin, step, shape, density):
    got = renderer.mass_from_moments(m, origin, step, density, raw=True)
    want = M.from_moments(m, origin, step, density)
    tol = M.tolerances(want, origin, step, shape)
    for e in range(_ffi.RM_MASS_PROPS):
        print("%-5s got %.17g want %.17g tol %.3g" % (PROP_NAMES[e], got[e], want[e], tol[e]))
    for e in range(_ffi.RM_MASS_PROPS):
        if np.isinf(want[e]):
            assert got[e] == want[e], PROP_NAMES[e]
        else:
            assert abs(got[e] - want[e]) <= tol[e], (PROP_NAMES[e], got[e], want[e], tol[e])
    return got


def test_from_moments_of_a_box_is_exact_where_it_must_be():
    lo, hi = (3, 10, 0), (40, 17, 25)
    m = M.box_moments(lo, hi)
    k, j, i = np.meshgrid(np.arange(lo[2], hi[2]), np.arange(lo[1], hi[1]), np.arange(lo[0], hi[0]), indexing="ij")
    assert m == M.moments_of_indices(i, j, k)                                  # the closed form is the enumeration
    origin, step, shape = (-1.0, 0.5, 2.0), (0.25, 0.125, 0.5), (48, 32, 25)      # powers of two: every product below is exact
    got = check_from_moments(m, origin, step, shape, 2.0)
    n = [hi[a] - lo[a] for a in range(3)]
    ext = [n[a] * step[a] for a in range(3)]
    vol = ext[0] * ext[1] * ext[2]
    assert got[_ffi.RM_MASS_VOLUME] == vol and got[_ffi.RM_MASS_MASS] == 2.0 * vol
    for a in range(3):
        assert got[_ffi.RM_MASS_CX + a] == origin[a] + step[a] * (lo[a] + hi[a] - 1) / 2.0
        assert got[_ffi.RM_MASS_LO_X + a] == origin[a] + lo[a] * step[a] and got[_ffi.RM_MASS_HI_X + a] == origin[a] + (hi[a] - 1) * step[a]
    assert got[_ffi.RM_MASS_IXY] == 0.0 and got[_ffi.RM_MASS_IYZ] == 0.0 and got[_ffi.RM_MASS_IXZ] == 0.0   # D_ab = 0 exactly
    # a box of cells: mass (b^2 + c^2) / 12 with the cells' full extents
    assert got[_ffi.RM_MASS_IXX] == pytest.approx(2.0 * vol * (ext[1] ** 2 + ext[2] ** 2) / 12.0, rel=1e-14)
    assert got[_ffi.RM_MASS_IZZ] == pytest.approx(2.0 * vol * (ext[0] ** 2 + ext[1] ** 2) / 12.0, rel=1e-14)


def sphere_lattice():
    cc, w = T.words_of((0, [0.0, 0.0, 0.0, 1.0]))
    n = 64
    return cc, w, (-1.5,) * 3, (F(3.0) / F(n - 1),) * 3, (n, n, n)


def test_from_moments_of_a_sphere_and_the_quadrature_bound():
    cc, w, origin, step, shape = sphere_lattice()
    m = M.lattice_moments(cc, w, origin, step, shape, 0.0)
    got = check_from_moments(m, origin, step, shape, 7.85)
    h = float(step[0])
    print("N = %d, N dV = %.9g, 4 pi / 3 = %.9g, bound %.3g" % (m[0], m[0] * h ** 3, 4.0 * math.pi / 3.0, 4.0 * math.pi * math.sqrt(3.0) * h))
    assert abs(m[0] * h ** 3 - 4.0 * math.pi / 3.0) <= 4.0 * math.pi * math.sqrt(3.0) * h      # surface area x sqrt(3) step
    assert got[_ffi.RM_MASS_VOLUME] == pytest.approx(m[0] * h ** 3, rel=1e-12)
    assert np.all(np.abs(got[_ffi.RM_MASS_CX:_ffi.RM_MASS_CZ + 1]) < h)          # a centred sphere
    assert got[_ffi.RM_MASS_IXX] == pytest.approx(0.4 * got[_ffi.RM_MASS_MASS], rel=0.05)   # 2/5 m r^2, to first order


@pytest.mark.parametrize("seed", range(10))
def test_from_moments_of_random_sets_on_a_4096_wide_lattice(seed):
    """Even seeds: 5000 random points.  Odd seeds: two disjoint boxes of up to 2^35 points in closed form, so N S_ab and S_a S_b
    reach 2^95 and their difference needs the 128-bit path."""
    rng = np.random.default_rng(1700 + seed)
    if seed % 2 == 0:
        i, j, k = rng.integers(0, 4096, (3, 5000))
        m = M.moments_of_indices(i, j, k)
    else:
        cut = int(rng.integers(1000, 3000))
        lo1, hi1 = [int(x) for x in rng.integers(0, 500, 3)], [cut] + [int(x) for x in rng.integers(3000, 4097, 2)]
        lo2, hi2 = [cut + int(rng.integers(1, 50))] + [int(x) for x in rng.integers(0, 2000, 2)], [int(x) for x in rng.integers(3500, 4097, 3)]
        m1, m2 = M.box_moments(lo1, hi1), M.box_moments(lo2, hi2)
        m = [a + b for a, b in zip(m1[:10], m2[:10])] + [min(a, b) for a, b in zip(m1[10:13], m2[10:13])] \
            + [max(a, b) for a, b in zip(m1[13:], m2[13:])]
        assert m[0] > 2 ** 33 and max(m[4:10]) > 2 ** 55 and max(m) < 2 ** 60
    origin = tuple(float(x) for x in rng.uniform(-900.0, 900.0, 3))
    step = tuple(float(x) for x in rng.uniform(1e-3, 0.3, 3))
    check_from_moments(m, origin, step, (4096,) * 3, float(rng.uniform(0.1, 20.0)))


def test_from_moments_of_an_empty_solid():
    got = check_from_moments([0] * 10 + [0xFFFFFFFF] * 3 + [0] * 3, (0.0, 1.0, 2.0), (0.1, 0.1, 0.1), (8, 8, 8), 3.0)
    assert np.all(got[:11] == 0.0) and np.all(got[11:14] == np.inf) and np.all(got[14:] == -np.inf)
    p = renderer.mass_from_moments([0] * 10 + [0xFFFFFFFF] * 3 + [0] * 3, (0.0, 1.0, 2.0), (0.1, 0.1, 0.1))
    assert p["volume"] == 0.0 and p["inertia"].shape == (3, 3) and np.all(p["bbox_lo"] == np.inf)


def test_from_moments_rejects_bad_arguments():
    L = _ffi.hip_lib()
    m = (C.c_uint64 * 16)(*M.box_moments((0, 0, 0), (4, 4, 4)))
    out = (C.c_double * 17)()
    o, s = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    assert L.rm_mass_from_moments(m, 16, o, s, 1.0, out, 17) == _ffi.RM_OK
    assert L.rm_mass_from_moments(None, 16, o, s, 1.0, out, 17) == _ffi.RM_ERR_NULL
    assert L.rm_mass_from_moments(m, 16, None, s, 1.0, out, 17) == _ffi.RM_ERR_NULL
    assert L.rm_mass_from_moments(m, 16, o, None, 1.0, out, 17) == _ffi.RM_ERR_NULL
    assert L.rm_mass_from_moments(m, 16, o, s, 1.0, None, 17) == _ffi.RM_ERR_NULL
    assert L.rm_mass_from_moments(m, 15, o, s, 1.0, out, 17) == _ffi.RM_ERR_ARG
    assert L.rm_mass_from_moments(m, 16, o, s, 1.0, out, 16) == _ffi.RM_ERR_ARG
    for density in (np.nan, np.inf, -np.inf):
        assert L.rm_mass_from_moments(m, 16, o, s, density, out, 17) == _ffi.RM_ERR_ARG
    for bad in ((1, 0, 1), (1, -1, 1), (np.inf, 1, 1), (1, 1, np.nan)):
        assert L.rm_mass_from_moments(m, 16, o, (C.c_float * 3)(*bad), 1.0, out, 17) == _ffi.RM_ERR_ARG, bad
    with pytest.raises(_ffi.RmError):
        renderer.mass_from_moments(list(m), (0, 0, 0), (1, 0, 1))
    with pytest.raises(ValueError):
        renderer.mass_from_moments(list(m), (0, 0), (1, 1, 1))


# ---- the brick classes ------------------------------------------------------------------------------------------------------------
def class_cases():
    return [(name, level) for name in MESH_SCENES for level in (0.0, 0.05)] + [("far " + label, 0.0) for label in B.far_lattices()]


@pytest.mark.parametrize("what, level", class_cases())
def test_the_class_model_never_clears_a_brick_whose_own_points_are_mixed(oracle, what, level):
    """Section 15 proves a cleared brick's TILE one-sided; its own points are a subset.  Checked on the oracle's lattice: every
    cleared brick's own points are all inside (class inside) or all outside, and the moments follow from the classes."""
    if what.startswith("far "):
        cc, w = B.far_program()
        origin, step, shape = B.far_lattices()[what[4:]]
    else:
        cc, w = oracle.serialize(*B.ALL_SCENES[what]())
        n = 72
        origin, step, shape = (-3.0,) * 3, (F(6.0) / F(n - 1),) * 3, (n, n, n)
    L, E = B.program_bound(cc, w, sparse_ref.lattice_P(origin, step, shape))
    keep, inside, stats = M.class_model(cc, w, origin, step, shape, level, L, E, MAX_DIST)
    points = M.lattice_inside(cc, w, origin, step, shape, level, MAX_DIST)
    mixed, full = M.own_points_mixed(points)
    print("%s level %g: %s" % (what, level, stats))
    assert not np.any(mixed & ~keep), "a cleared brick has own points on both sides"
    assert np.all(full[inside]), "a brick classed inside has an outside point"
    assert not np.any((full | mixed) & ~keep & ~inside), "a brick classed outside has an inside point"
    assert stats["bricks"] <= stats["evaluations"] <= stats["bricks"] + 512 * stats["bricks_kept"]
    # the moments from the classes: closed form for inside bricks, enumeration for kept ones
    total = [0] * 10 + [M.NO_MIN] * 3 + [0] * 3
    for kb, jb, ib in zip(*np.nonzero(inside | keep)):
        lo = (8 * ib, 8 * jb, 8 * kb)
        hi = tuple(min(lo[a] + 8, shape[a]) for a in range(3))
        if inside[kb, jb, ib]:
            m = M.box_moments(lo, hi)
        else:
            m = M.moments_of_inside(points[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]], lo)
        total = [a + b for a, b in zip(total[:10], m[:10])] + [min(a, b) for a, b in zip(total[10:13], m[10:13])] \
            + [max(a, b) for a, b in zip(total[13:], m[13:])]
    assert total == M.moments_of_inside(points)


def test_the_class_model_finds_inside_bricks():
    """The counts the GPU tests expect (tests/test_gpu_mass.py): inside bricks must occur, or the closed form goes untested."""
    cc, w = T.words_of((0, [0.0, 0.0, 0.0, 2.5]))
    for origin, step, shape, want in (((-3.0,) * 3, (F(6.0) / F(71),) * 3, (72,) * 3, (317, 90, 322)),
                                      ((-3.0, -2.5, -2.0), (0.09, 0.11, 0.1), (61, 47, 39), (159, 52, 29))):
        L, E = B.program_bound(cc, w, sparse_ref.lattice_P(origin, step, shape))
        keep, inside, stats = M.class_model(cc, w, origin, step, shape, 0.0, L, E, MAX_DIST)
        outside = stats["bricks"] - stats["bricks_kept"] - stats["bricks_inside"]
        assert (stats["bricks_kept"], stats["bricks_inside"], outside) == want, stats
