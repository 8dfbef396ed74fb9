"""Surface measures without a GPU: the contract's restatement tests/surface_ref.py against independent
restatements of other contracts (topology_ref's edges, support_ref's runs and landings), its orientation, closed forms, the
direction weights against a quadrature, the accuracy of AREA on balls, and the host functions rm_surface_measures and
rm_surface_directions of the library (no context, no GPU)."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import support_ref
import surface_ref as SR
import topology_ref
from ray_marching_amd import _ffi, renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = (1.0, 1.0, 1.0)


def random_occupancy(seed, shape=(9, 11, 13), p=0.55):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


# ---- pair identities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_axis_pairs_of_the_solid_are_the_edges(seed):
    occ = random_occupancy(seed)
    P = SR.pairs(SR.counts(occ))
    assert int(P[1, 1, 0:3].sum()) == topology_ref.topology(occ != 0)["counts"]["edges"]
    assert int(SR.points(SR.counts(occ))[1]) == int(occ.sum()) and int(SR.points(SR.counts(occ)).sum()) == occ.size


@pytest.mark.parametrize("up", ["+z", "-z", "+x", "-y"])
@pytest.mark.parametrize("seed", range(2))
def test_runs_and_landings_are_pairs_of_the_support_mask(seed, up):
    occ = random_occupancy(10 + seed)
    mask, counts, _ = support_ref.layerwise(occ, up, r2=1, plate=None)
    P = SR.pairs(SR.counts(mask))
    axis, neg = divmod(support_ref.up_index(up), 2)
    pair = (lambda lo, hi: int(P[hi, lo, axis])) if neg else (lambda lo, hi: int(P[lo, hi, axis]))   # (lower point, the one above it)
    assert sum(pair(s, support_ref.OVERHANG) for s in (3, 4)) == counts["runs"]
    assert sum(pair(a, s) for a in (1, 2) for s in (3, 4)) == counts["landings"]


# ---- orientation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", range(3))
def test_mirroring_exchanges_the_ends(axis):
    data = np.random.default_rng(20 + axis).integers(0, 8, size=(6, 7, 8), dtype=np.uint8)
    mirrored = np.flip(data, axis=2 - axis)                      # [k, j, i]
    P, Q = SR.pairs(SR.counts(data)), SR.pairs(SR.counts(mirrored))
    for nu, d in enumerate(SR.DIRECTIONS):
        m = list(d)
        m[axis] = -m[axis]
        if tuple(m) in SR.DIRECTIONS:                            # (no component along the axis: the pair keeps its order)
            assert np.array_equal(Q[:, :, SR.DIRECTIONS.index(tuple(m))], P[:, :, nu])
        else:
            assert np.array_equal(Q[:, :, SR.DIRECTIONS.index(tuple(-x for x in m))], P[:, :, nu].T)
    a, b = SR.measures(SR.counts(data), UNIT, [1, 2], [0, 5]), SR.measures(SR.counts(mirrored), UNIT, [1, 2], [0, 5])
    name = "xyz"[axis]
    assert a["facet_pos_" + name] == b["facet_neg_" + name] and a["facet_neg_" + name] == b["facet_pos_" + name]
    for other in "xyz".replace(name, ""):
        assert a["facet_pos_" + other] == b["facet_pos_" + other] and a["facet_neg_" + other] == b["facet_neg_" + other]
    assert a["area"] == pytest.approx(b["area"], rel=1e-14)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
def test_full_lattice_has_only_padding_pairs():
    nz, ny, nx = 4, 5, 6
    w = SR.counts(np.ones((nz, ny, nx), dtype=np.uint8))
    P = SR.pairs(w)
    assert int(P[1, 0].sum()) + int(P[0, 1].sum()) + int(P[1, 1].sum()) == int(P.sum()) and int(P[0, 0].sum()) == 0
    assert [int(P[1, 0, k]) for k in range(3)] == [ny * nz, nx * nz, nx * ny] and [int(P[0, 1, k]) for k in range(3)] == [ny * nz, nx * nz, nx * ny]
    assert SR.measures(w, (0.5, 0.5, 0.5), [1], [0])["facet_area"] == 2 * (nx * ny + ny * nz + nx * nz) * 0.25


def test_one_point_has_26_crossings():
    occ = np.zeros((3, 4, 5), dtype=np.uint8)
    occ[1, 2, 3] = 1
    P = SR.pairs(SR.counts(occ))
    assert np.array_equal(P[1, 0], np.ones(13, dtype=np.uint64)) and np.array_equal(P[0, 1], np.ones(13, dtype=np.uint64))
    assert int(P.sum()) == 26


@pytest.mark.parametrize("abc", [(1, 1, 1), (2, 3, 4), (5, 1, 3)])
def test_box_facet_area(abc):
    a, b, c = abc
    occ = np.zeros((c + 3, b + 2, a + 4), dtype=np.uint8)
    occ[1:1 + c, 2:2 + b, 0:a] = 1                               # (touches the border on -x: the padding closes it)
    m = SR.measures(SR.counts(occ), (0.25, 0.25, 0.25), [1], [0])
    assert m["facet_area"] == 2 * (a * b + b * c + c * a) * 0.0625
    assert (m["facet_pos_x"], m["facet_pos_y"], m["facet_pos_z"]) == (b * c * 0.0625, a * c * 0.0625, a * b * 0.0625)
    anis = SR.measures(SR.counts(occ), (0.5, 0.25, 2.0), [1], [0])
    assert anis["facet_pos_x"] == b * c * 0.5 and anis["facet_neg_z"] == a * b * 0.125 and math.isnan(anis["area"])


# ---- the weights ----------------------------------------------------------------------------------------------------------------------
def test_weights_sum_to_one_and_match_a_quadrature():
    w1, w2, w3 = SR.WEIGHTS
    assert abs(3.0 * w1 + 6.0 * w2 + 4.0 * w3 - 1.0) < 1e-12
    coarse, fine = SR.weights_quadrature(200), SR.weights_quadrature(400)
    for w, c, f in zip(SR.WEIGHTS, coarse, fine):
        assert abs(f - w) <= abs(f - c) + 1e-12, (w, c, f)       # within the change between the two grids
    # the Monte-Carlo figures of the prototype (+-2e-4)
    assert abs(w1 - 0.0916) < 4e-4 and abs(w2 - 0.0740) < 4e-4 and abs(w3 - 0.0703) < 4e-4


def test_the_library_and_the_script_carry_the_same_weights():
    src = open(os.path.join(ROOT, "ray-marching_amd", "csrc", "rm_abi.hip")).read()
    m = re.search(r"kSurfWeight\[3\] = \{([^}]*)\}", src)
    assert m and tuple(float(x) for x in m.group(1).split(",")) == SR.WEIGHTS
    import importlib.util
    spec = importlib.util.spec_from_file_location("surface_weights", os.path.join(ROOT, "tools", "surface_weights.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert tuple(float("%.17g" % x) for x in mod.weights()) == SR.WEIGHTS


# ---- the accuracy of AREA ---------------------------------------------------------------------------------------------------------------
# Recorded with the committed weights: per radius the largest |AREA / 4 pi R^2 - 1| over BALL_CENTRES.  The
# test bounds each radius by twice its record.
BALL_CENTRES = ((0.37, 0.21, 0.13), (0.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.25, 0.4, 0.1), (0.5, 0.0, 0.0), (0.11, 0.47, 0.33))
BALL_RECORD = {6.0: 0.0347, 10.3: 0.0108, 14.7: 0.0064, 20.2: 0.0011}


@pytest.mark.parametrize("radius", sorted(BALL_RECORD))
def test_area_of_balls(radius):
    worst = 0.0
    for centre in BALL_CENTRES:
        m = SR.measures(SR.counts(SR.ball(radius, centre)), UNIT, [1], [0])
        err = m["area"] / (4.0 * math.pi * radius * radius) - 1.0
        print("R %.1f centre %s: %+.4f %%" % (radius, centre, 100.0 * err))
        worst = max(worst, abs(err))
    assert worst <= 2.0 * BALL_RECORD[radius]


def test_area_of_a_cube_is_the_worst_case():
    occ = np.zeros((14, 14, 14), dtype=np.uint8)
    occ[2:12, 2:12, 2:12] = 1
    m = SR.measures(SR.counts(occ), UNIT, [1], [0])
    assert m["facet_area"] == 600.0 and -0.14 < m["area"] / 600.0 - 1.0 < -0.12


# ---- the library's host functions ------------------------------------------------------------------------------------------------------
def test_directions():
    assert [tuple(int(x) for x in d) for d in renderer.surface_directions()] == list(SR.DIRECTIONS)
    L = _ffi.hip_lib()
    import ctypes as C
    out = (C.c_int * 39)()
    assert L.rm_surface_directions(None, 39) == _ffi.RM_ERR_NULL and L.rm_surface_directions(out, 38) == _ffi.RM_ERR_ARG


@pytest.mark.parametrize("step", [(1.0, 1.0, 1.0), (0.125, 0.125, 0.125), (0.3, 0.3, 0.3), (0.5, 0.25, 2.0)])
def test_library_measures_equal_the_restatement(step):
    rng = np.random.default_rng(5)
    for data in (rng.integers(0, 8, size=(7, 6, 9), dtype=np.uint8), SR.ball(5.2, (0.3, 0.1, 0.2))):
        w = SR.counts(data)
        for A, B in (([1], [0]), ([1, 2], [3, 4]), ([0], [1, 7]), ([5], [2])):
            got, ref = renderer.surface_measures(w, step, A, B), SR.measures(w, step, A, B)
            assert tuple(got) == SR.MEASURE_NAMES
            for name in SR.MEASURE_NAMES:
                if math.isnan(ref[name]):
                    assert math.isnan(got[name])
                else:
                    assert got[name] == pytest.approx(ref[name], rel=1e-14, abs=0.0), name   # (the same operations in binary64)


def test_measures_argument_errors():
    import ctypes as C
    L = _ffi.hip_lib()
    w = np.zeros(SR.COUNTS, dtype=np.uint64)
    wp = w.ctypes.data_as(C.POINTER(C.c_uint64))
    out = np.full(_ffi.RM_SURF_MEASURES, -1.0)
    op = out.ctypes.data_as(C.POINTER(C.c_double))
    st = lambda *s: np.array(s, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    good = np.ones(3, dtype=np.float32)
    gp = good.ctypes.data_as(C.POINTER(C.c_float))
    assert L.rm_surface_measures(wp, 840, gp, 2, 1, op, 8) == _ffi.RM_OK and np.all(out == 0.0)
    out[:] = -1.0
    for args, status in (((wp, 840, gp, 3, 1, op, 8), _ffi.RM_ERR_ARG),            # overlapping masks
                         ((wp, 840, gp, 0, 1, op, 8), _ffi.RM_ERR_ARG),            # an empty mask
                         ((wp, 840, gp, 2, 0, op, 8), _ffi.RM_ERR_ARG),
                         ((wp, 840, gp, 2, 256, op, 8), _ffi.RM_ERR_ARG),          # a ninth class
                         ((wp, 839, gp, 2, 1, op, 8), _ffi.RM_ERR_ARG),            # short arrays
                         ((wp, 840, gp, 2, 1, op, 7), _ffi.RM_ERR_ARG),
                         ((wp, 840, st(1.0, 0.0, 1.0), 2, 1, op, 8), _ffi.RM_ERR_ARG),
                         ((wp, 840, st(1.0, -1.0, 1.0), 2, 1, op, 8), _ffi.RM_ERR_ARG),
                         ((wp, 840, st(np.inf, 1.0, 1.0), 2, 1, op, 8), _ffi.RM_ERR_ARG),
                         ((wp, 840, st(1.0, 1.0, np.nan), 2, 1, op, 8), _ffi.RM_ERR_ARG),
                         ((None, 840, gp, 2, 1, op, 8), _ffi.RM_ERR_NULL),
                         ((wp, 840, None, 2, 1, op, 8), _ffi.RM_ERR_NULL),
                         ((wp, 840, gp, 2, 1, None, 8), _ffi.RM_ERR_NULL)):
        assert L.rm_surface_measures(*args) == status, args[1:]
        assert np.all(out == -1.0)
    with pytest.raises(ValueError):
        renderer.surface_measures(w, good, [8], [0])
    with pytest.raises(_ffi.RmError):
        renderer.surface_measures(w, good, [1], [1, 2])


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "rm_abi.h")).read()
    for k, name in enumerate(_ffi.SURF_MEASURE_NAMES):
        m = re.search(r"\bRM_SURF_%s = (\d+)" % name.upper(), text)
        assert m and int(m.group(1)) == k, name
    for k, name in enumerate(_ffi.SURF_STAT_NAMES):
        m = re.search(r"\bRM_SURF_STAT_%s = (\d+)" % name.upper(), text)
        assert m and int(m.group(1)) == k, name
    for name, value in (("CLASSES", 8), ("DIRS", 13), ("POINTS", 0), ("PAIRS", 8), ("COUNTS", 840), ("STATS", 5), ("MEASURES", 8)):
        assert re.search(r"\bRM_SURF_%s = %d\b" % (name, value), text) and getattr(_ffi, "RM_SURF_" + name) == value
    assert _ffi.RM_SURF_PAIR(7, 7, 12) == 839 == SR.pair_index(7, 7, 12) and _ffi.RM_SURF_PAIR(0, 0, 0) == 8
    assert "8 + (8 * (int)(a) + (int)(b)) * 13 + (int)(nu)" in text
    assert _ffi.SURF_MEASURE_NAMES == SR.MEASURE_NAMES


def test_surface_layout_check(tmp_path):
    """tests/cpp/surface_layout_check.cpp under ASan + UBSan: rml::SurfScratch and rml::SurfTileLds against offsets written out by
    hand, and a walk over the tiles as the kernel indexes them."""
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    exe = tmp_path / "surface_layout_check"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"), "-o", str(exe),
                            os.path.join(ROOT, "tests", "cpp", "surface_layout_check.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "surface layout ok" in run.stdout


def test_tool_gates():
    from ray_marching_amd import surface
    assert surface.parse_gates("area>12.5, contact>0") == [("area", 12.5), ("contact", 0.0)]
    assert surface.parse_gates("") == []
    for bad in ("area", "volume>1", "area<1", "area>x", "contact>"):
        with pytest.raises(ValueError):
            surface.parse_gates(bad)
