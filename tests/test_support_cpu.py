"""The yardstick of the overhang-and-support tests (tests/support_ref.py), checked without a GPU: its two
forms against each other, closed forms, invariants; the scratch and LDS layouts under ASan + UBSan; the conversion from an angle to
a squared reach; the command line's gate parser and its choice of the best direction."""
import numpy as np
import pytest

import support_ref as SR

SHAPE = (5, 6, 7)                                                # (nz, ny, nx): 7 x 6 x 5 points
DENSITIES = (0.1, 0.4, 0.8)


def random_occ(shape, density, seed=0):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def equal(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("plate", [None, 0, 2])
@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("up", SR.UPS)
def test_per_point_equals_layerwise(up, density, plate):
    for r2 in (0, 1, 2, 5):
        occ = random_occ(SHAPE, density, seed=int(density * 10) + r2 + 7 * SR.up_index(up))
        a, b = SR.per_point(occ, up, r2, plate), SR.layerwise(occ, up, r2, plate)
        assert equal(a, b), (up, density, plate, r2)
        mask, counts, profile = b
        assert mask.dtype == np.uint8 and mask.shape == occ.shape and profile.shape == (occ.shape[2 - (SR.up_index(up) >> 1)], 4)
        # the invariants: overhangs are inside, supports outside; each profile column sums to its count
        assert np.array_equal((mask == 1) | (mask == 2), occ != 0)
        assert [int(profile[:, k].sum()) for k in range(4)] == [counts[k] for k in ("points", "overhang", "support_on_plate", "support_on_part")]
        assert counts["base"] == int(profile[counts["plate"], 0]) and not profile[:counts["plate"], 1:].any()
        assert counts["runs"] <= counts["overhang"] and counts["landings"] <= counts["runs"]
        if plate is None and occ.any():
            assert counts["base"] > 0 and not profile[:counts["plate"], 0].any()


@pytest.mark.parametrize("up", ["+z", "-y", "+x"])
def test_wide_discs(up):
    for r2 in (9, 25, 255):
        occ = random_occ((12, 12, 12), 0.04, seed=r2)
        assert equal(SR.per_point(occ, up, r2), SR.layerwise(occ, up, r2)), (up, r2)


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("up", SR.UPS)
def test_support_is_monotone_in_the_reach(up, density):
    occ = random_occ((9, 8, 10), density, seed=3)
    last = None
    for r2 in (0, 1, 2, 4, 5, 9, 255):
        mask, counts, _ = SR.layerwise(occ, up, r2)
        now = (mask == 2), (mask >= 3)
        if last is not None:
            assert not np.any(now[0] & ~last[0]) and not np.any(now[1] & ~last[1])     # a wider disc supports more: subsets
        last = now


def test_the_empty_and_the_full_lattice():
    for up in SR.UPS:
        mask, counts, profile = SR.layerwise(np.zeros(SHAPE, dtype=np.uint8), up, 1)
        assert counts == dict.fromkeys(SR.COUNT_NAMES, 0) and not mask.any() and not profile.any()
        mask, counts, profile = SR.layerwise(np.ones(SHAPE, dtype=np.uint8), up, 0)
        assert np.all(mask == 1) and counts["overhang"] == counts["support_on_plate"] == counts["support_on_part"] == 0


@pytest.mark.parametrize("r2", sorted(SR.TABLE_OVERHANG))
def test_table(r2):
    """The top's lower layer has 10 x 8 points; the disc of r2 around the 2 x 2 leg covers 4, 12, 16, 24 of them."""
    occ = SR.table()
    n = SR.TABLE_OVERHANG[r2]
    covered = sum(1 for i in range(1, 11) for j in range(1, 9)
                  if any((i - a) ** 2 + (j - b) ** 2 <= r2 for a in (5, 6) for b in (4, 5)))
    assert n == 80 - covered
    for form in (SR.per_point, SR.layerwise):
        mask, counts, profile = form(occ, "+z", r2)
        assert counts == {"points": 184, "plate": 0, "base": 4, "overhang": n, "support_on_plate": 6 * n, "support_on_part": 0, "runs": n,
                          "landings": 0}
        assert np.all(mask[7] == occ[7]) and np.count_nonzero(mask[6] == 2) == n and np.all(profile[:6, 2] == n)
        mask, counts, _ = form(occ, "-z", r2)
        assert counts == {"points": 184, "plate": 1, "base": 80, "overhang": 0, "support_on_plate": 0, "support_on_part": 0, "runs": 0,
                          "landings": 0}
        assert np.array_equal(mask, occ)


def test_shelf_lands_on_the_part():
    """A base slab, a post and a shelf: the shelf's a x b = 9 x 7 points overhang at r2 = 0 but for the p = 4 over the post; every
    support column is g = 5 points high (the gap between slab and shelf) and stands on the slab: SUPPORT_ON_PART = g (a b - p),
    RUNS = LANDINGS = a b - p, SUPPORT_ON_PLATE = 0."""
    occ = SR.shelf()
    a, b, p, g = 9, 7, 4, 5
    for form in (SR.per_point, SR.layerwise):
        mask, counts, profile = form(occ, "+z", 0)
        assert counts == {"points": 16 * 12 * 2 + p * g + a * b, "plate": 1, "base": 16 * 12, "overhang": a * b - p, "support_on_plate": 0,
                          "support_on_part": g * (a * b - p), "runs": a * b - p, "landings": a * b - p}
        assert np.all(mask[0] == 0) and set(np.unique(mask[3:8])) == {0, 1, 4}
    # with the plate under the slab's margin the slab overhangs too, and its supports stand on the plate
    _, counts, _ = SR.layerwise(occ, "+z", 0, plate=0)
    assert counts["support_on_plate"] == 16 * 12 and counts["overhang"] == 16 * 12 + a * b - p and counts["landings"] == a * b - p


def test_support_layout_check(tmp_path):
    """tests/cpp/support_layout_check.cpp under ASan + UBSan: rml::SupportScratch, rml::SupportProfile and rml::SupCoverLds against
    offsets written out by hand."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    exe = tmp_path / "support_layout_check"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(root, "include"), "-I", os.path.join(root, "ray-marching_amd", "csrc"), "-o", str(exe),
                            os.path.join(root, "tests", "cpp", "support_layout_check.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "support layout ok" in run.stdout


def test_angles_to_squared_reaches():
    from ray_marching_amd import renderer
    r2 = renderer.reach_r2
    assert r2(45.0, 0.1, 0.1) == 1 and r2(45.0, 0.1, (0.1, 0.1)) == 1       # tan(45 degrees) is just below 1 in binary64
    assert r2(0.0, 0.1, 0.1) == 0 and r2(44.9, 0.1, 0.1) == 0
    assert r2(float(np.degrees(np.arctan(2.0))), 0.1, 0.1) == 4
    assert r2(45.0, 0.2, 0.1) == 4 and r2(45.0, 0.1, 0.2) == 0              # taller layers reach further, in points
    assert r2(60.0, 1.0, 1.0) == 3 and r2(86.0, 1.0, 1.0) == 204
    for bad in (-1.0, 90.0, 120.0, float("nan")):
        with pytest.raises(ValueError):
            r2(bad, 0.1, 0.1)
    for bad_in in ((0.1, 0.2), (0.1, 0.1, 0.1), 0.0, -1.0):
        with pytest.raises(ValueError):
            r2(45.0, 0.1, bad_in)
    with pytest.raises(ValueError):
        r2(45.0, 0.0, 0.1)
    with pytest.raises(ValueError):
        r2(87.0, 1.0, 1.0)                                                  # tan^2 = 364 > 255


def test_printability_gates():
    from ray_marching_amd import supports
    assert supports.parse_gates("overhang>0, support>2.5,landings>10") == [("overhang", 0.0), ("support", 2.5), ("landings", 10.0)]
    assert supports.parse_gates("") == []
    for bad in ("overhang", "volume>1", "overhang<1", "support>x", "landings>"):
        with pytest.raises(ValueError):
            supports.parse_gates(bad)
    values = {"overhang": 3, "support": 2.5, "landings": 0}
    assert supports.failed_gates(supports.parse_gates("overhang>0,support>2.5,landings>0"), values) == ["overhang = 3 > 0"]
    assert supports.failed_gates(supports.parse_gates("support>2.4"), values) == ["support = 2.5 > 2.4"]


def test_best_direction_tie_breaks():
    from ray_marching_amd import supports
    def reports(**over):
        r = {up: {"support": 5.0, "landings": 7} for up in supports.BEST_ORDER}
        for up, (s, l) in over.items():
            r[{"pz": "+z", "nz": "-z", "py": "+y", "ny": "-y", "px": "+x", "nx": "-x"}[up]] = {"support": s, "landings": l}
        return r
    assert supports.BEST_ORDER == ("+z", "-z", "+y", "-y", "+x", "-x")
    assert supports.best_direction(reports()) == "+z"                               # all equal: the order
    assert supports.best_direction(reports(nx=(4.0, 100))) == "-x"                  # the least support volume wins over landings
    assert supports.best_direction(reports(ny=(5.0, 6), px=(5.0, 6))) == "-y"       # fewer landings, then the order
    assert supports.best_direction(reports(pz=(5.0, 8), nz=(5.0, 8))) == "+y"
