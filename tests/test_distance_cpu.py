"""The yardstick of the distance-transform tests (tests/distance_ref.py), checked without a GPU: its two
forms against each other, closed forms, the algebra of the opening; the scratch layouts under ASan + UBSan; the command line's
gate parser and the conversion from world widths to squared radii."""
import numpy as np
import pytest

import distance_ref as DR

RANDOM_CASES = [(shape, density) for shape in ((9, 5, 7), (12, 12, 12)) for density in (0.05, 0.5, 0.95)]   # (nz, ny, nx): 7x5x9


def random_occ(shape, density, seed=0):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def all_cases():
    for shape, density in RANDOM_CASES:
        yield "%s at %g" % (shape, density), random_occ(shape, density, seed=int(density * 100) + shape[0])
    for shape in ((9, 5, 7), (12, 12, 12)):
        yield "%s empty" % (shape,), np.zeros(shape, dtype=np.uint8)
        yield "%s full" % (shape,), np.ones(shape, dtype=np.uint8)


@pytest.mark.parametrize("what,occ", list(all_cases()), ids=[w for w, _ in all_cases()])
def test_brute_equals_separable(what, occ):
    b, s = DR.brute(occ), DR.separable(occ)
    assert b.dtype == np.uint32 and b.shape == occ.shape
    assert np.array_equal(b, s), what
    assert np.array_equal((b & DR.INSIDE_BIT) != 0, occ != 0)
    d = b & DR.NONE
    if occ.any():
        assert d.min() >= 1 and d.max() < 3 * 1023 ** 2
        assert np.all(d[occ != 0] <= DR.layer_bound(occ.shape)[occ != 0])
    else:
        assert np.all(b == DR.NONE)
        assert DR.counts(b) == {"points": 0, "max_inside": 0, "argmax_inside": DR.NO_INDEX, "max_outside": DR.NONE, "argmax_outside": 0}


@pytest.mark.parametrize("shape", [(4, 3, 5), (9, 5, 7), (2, 2, 2), (3, 2, 40)])
def test_full_lattice_closed_form(shape):
    """A full a x b x c lattice: D2 = min(i + 1, a - i, ...)^2, and nothing is outside."""
    full = np.ones(shape, dtype=np.uint8)
    want = DR.layer_bound(shape)
    for v in (DR.brute(full), DR.separable(full)):
        assert np.array_equal(v, want.astype(np.uint32) | np.uint32(DR.INSIDE_BIT))
    c = DR.counts(DR.separable(full))
    assert c["points"] == full.size and c["max_outside"] == 0 and c["argmax_outside"] == DR.NO_INDEX
    assert c["max_inside"] == int(want.max()) and c["argmax_inside"] == int(np.flatnonzero(want.ravel() == want.max())[0])


@pytest.mark.parametrize("shape,hole", [((9, 5, 7), (4, 2, 3)), ((12, 12, 12), (0, 11, 5)), ((3, 2, 40), (1, 0, 28))])
def test_single_outside_point_closed_form(shape, hole):
    """One outside point in a full lattice: the minimum of the layer's bound and the squared offset to the point."""
    occ = np.ones(shape, dtype=np.uint8)
    occ[hole] = 0
    k, j, i = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    off = (k - hole[0]) ** 2 + (j - hole[1]) ** 2 + (i - hole[2]) ** 2
    want = np.minimum(DR.layer_bound(shape), off).astype(np.uint32) | np.uint32(DR.INSIDE_BIT)
    want[hole] = 1                                                 # the outside point: its nearest inside point is a face neighbour
    assert np.array_equal(DR.brute(occ), want) and np.array_equal(DR.separable(occ), want)


@pytest.mark.parametrize("what,occ", list(all_cases()), ids=[w for w, _ in all_cases()])
@pytest.mark.parametrize("r2", [0, 1, 2, 4, 9])
def test_opening_is_anti_extensive_and_idempotent(what, occ, r2):
    inside = occ != 0
    mask, c = DR.features(occ, r2, r2)
    opened = mask == 1
    assert not np.any(opened & ~inside) and np.array_equal((mask == 1) | (mask == 2), inside)      # opened is a subset of the inside
    assert np.array_equal((mask == 0) | (mask == 3), ~inside)
    assert c["thin"] == np.count_nonzero(mask == 2) and c["narrow"] == np.count_nonzero(mask == 3)
    assert c["core"] <= np.count_nonzero(opened) and c["core"] + c["thin"] <= np.count_nonzero(inside)
    if r2 == 0:
        assert c["thin"] == 0 and c["narrow"] == 0 and c["core"] == np.count_nonzero(inside)
    # opening the opened set changes nothing: every point of it lies in a ball that fits
    again, c2 = DR.features(opened.astype(np.uint8), r2, None)
    assert c2["thin"] == 0 and np.array_equal(again == 1, opened), what
    # and the brute distance gives the same features as the separable one
    core = inside & ((DR.brute(occ) & DR.NONE).astype(np.int64) > r2)
    pts = np.stack(np.nonzero(np.ones(occ.shape, dtype=bool)), axis=1).astype(np.int64)
    far = DR.nearest_brute(pts, pts[core.ravel()]).reshape(occ.shape) > r2
    assert np.array_equal(mask == 2, inside & far), what


def test_skipped_half_leaves_its_classes():
    occ = random_occ((9, 5, 7), 0.5, seed=3)
    both, _ = DR.features(occ, 1, 1)
    wall, cw = DR.features(occ, 1, None)
    gap, cg = DR.features(occ, None, 1)
    assert set(np.unique(wall)) <= {0, 1, 2} and set(np.unique(gap)) <= {0, 1, 3}
    assert cw["gap_core"] == cw["narrow"] == 0 and cg["core"] == cg["thin"] == 0
    assert np.array_equal(wall == 2, both == 2) and np.array_equal(gap == 3, both == 3)


def test_distance_layout_check(tmp_path):
    """tests/cpp/distance_layout_check.cpp under ASan + UBSan: rml::DistScratch, rml::DistFeatureScratch and rml::DistColumnLds
    against offsets written out by hand."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    exe = tmp_path / "distance_layout_check"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(root, "include"), "-I", os.path.join(root, "ray-marching_amd", "csrc"), "-o", str(exe),
                            os.path.join(root, "tests", "cpp", "distance_layout_check.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "distance layout ok" in run.stdout


def test_printability_gates():
    from ray_marching_amd import thickness
    assert thickness.parse_gates("thin>0, narrow>10,inscribed<1.5") == [("thin", ">", 0.0), ("narrow", ">", 10.0), ("inscribed", "<", 1.5)]
    assert thickness.parse_gates("") == []
    for bad in ("thin", "volume>1", "thin<1", "inscribed>1", "thin>x", "inscribed<"):
        with pytest.raises(ValueError):
            thickness.parse_gates(bad)
    values = {"thin": 3, "narrow": 0, "inscribed": 1.25}
    gates = thickness.parse_gates("thin>0,narrow>0,inscribed<1.5")
    assert thickness.failed_gates(gates, values) == ["thin = 3 > 0", "inscribed = 1.25 < 1.5"]
    assert thickness.failed_gates(thickness.parse_gates("thin>3,inscribed<1.25"), values) == []


def test_world_widths_to_squared_radii():
    from ray_marching_amd import renderer
    r2 = renderer.squared_radius
    assert r2(0.8, 0.1) == 16 and r2(0.8, (0.1, 0.1, 0.1)) == 16       # a ball of radius 4 points
    assert r2(0.0, 0.1) == 0 and r2(0.19, 0.1) == 0 and r2(0.2, 0.1) == 1
    assert r2(0.5, 0.1) == 6                                            # floor(2.5^2)
    assert r2(1.0, np.float32(0.125)) == 16
    for bad_step in ((0.1, 0.1, 0.2), (0.1, 0.2), 0.0, -1.0):
        with pytest.raises(ValueError):
            r2(0.8, bad_step)
    for bad_width in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            r2(bad_width, 0.1)
