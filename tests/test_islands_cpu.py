"""The yardstick of the layer-regions-and-islands tests (tests/islands_ref.py), checked without a GPU: its
two forms against each other and against scipy.ndimage.label, closed forms, invariants, the overhang points of tests/support_ref.py
as a bound; the scratch and LDS layouts under ASan + UBSan; the root loop; the command line's gate parser and its choice of the
best direction."""
import numpy as np
import pytest

import islands_ref as IR
import support_ref as SR

SHAPE = (5, 6, 7)                                                # (nz, ny, nx): 7 x 6 x 5 points
DENSITIES = (0.1, 0.4, 0.8)


def random_occ(shape, density, seed=0):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def invariants(occ, up, r2, plate, r):
    """What holds for every Result."""
    a = SR.up_index(up) >> 1
    nh = occ.shape[2 - a]
    rows, c = r.rows, r.counts
    assert r.labels.dtype == np.uint32 and r.mask.dtype == np.uint8 and r.profile.shape == (nh, 4) and rows.shape == (c["regions"], 12)
    h0 = c["plate"]
    keys = list(zip(rows[:, IR.LAYER].tolist(), rows[:, IR.FIRST].tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)                  # numbered by (LAYER, FIRST)
    heights = np.indices(occ.shape)[2 - a]
    heights = nh - 1 - heights if SR.up_index(up) & 1 else heights
    inside = occ != 0
    assert int(rows[:, IR.POINTS].sum()) == np.count_nonzero(inside & (heights >= h0))
    assert np.array_equal(r.labels > 0, inside & (heights >= h0)) and np.array_equal(r.mask > 0, inside)
    assert [int(r.profile[:, k].sum()) for k in range(4)] == [c["points"], c["regions"], c["islands"], c["island_points"]]
    assert not r.profile[:h0, 1:].any() and c["base_regions"] == int(r.profile[h0, 1]) and c["max_layer_regions"] == int(r.profile[:, 1].max())
    assert np.all(rows[:, IR.SUPPORTED] <= rows[:, IR.POINTS]) and np.all(rows[:, IR.BELOW_MIN] <= rows[:, IR.BELOW_MAX])
    assert np.all(rows[:, IR.MIN_A] <= rows[:, IR.MAX_A]) and np.all(rows[:, IR.MIN_B] <= rows[:, IR.MAX_B])
    # a link goes to the layer below; an island is a region without a supported point, and the other way round
    linked = rows[:, IR.BELOW_MIN] > 0
    assert np.all(rows[rows[linked, IR.BELOW_MIN] - 1, IR.LAYER] == rows[linked, IR.LAYER] - 1)
    assert np.all(rows[rows[linked, IR.BELOW_MAX] - 1, IR.LAYER] == rows[linked, IR.LAYER] - 1)
    assert np.array_equal(rows[:, IR.SUPPORTED] == 0, (rows[:, IR.LAYER] > h0) & ~linked)
    # the first point carries the region's number, and the region lies in its bounding box
    first = rows[:, IR.FIRST].astype(np.int64)
    assert np.array_equal(r.labels.reshape(-1)[first], np.arange(1, len(rows) + 1))
    # island points are overhang points of the support restatement; no overhang, no island
    smask, scounts, _ = SR.layerwise(occ, up, r2, plate)
    assert not np.any((r.mask == 2) & (smask != 2)) and scounts["plate"] == h0 and scounts["points"] == c["points"]
    assert int(rows[:, IR.SUPPORTED].sum()) == int(rows[:, IR.POINTS].sum()) - scounts["overhang"]
    if scounts["overhang"] == 0:
        assert c["islands"] == 0
    root = IR.roots(rows)
    assert np.all((rows[root - 1, IR.BELOW_MIN] == 0)) and np.all(root <= np.arange(1, len(rows) + 1))


@pytest.mark.parametrize("plate", [None, 0, 2])
@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("up", SR.UPS)
def test_per_point_equals_layerwise(up, density, plate):
    for r2 in (0, 1, 2, 5):
        occ = random_occ(SHAPE, density, seed=int(density * 10) + r2 + 7 * SR.up_index(up))
        a, b = IR.per_point(occ, up, r2, plate), IR.layerwise(occ, up, r2, plate)
        assert IR.same(a, b), (up, density, plate, r2)
        invariants(occ, up, r2, plate, b)


@pytest.mark.parametrize("up", ["+z", "-y", "+x"])
def test_wide_discs(up):
    for r2 in (9, 25, 255):
        occ = random_occ((12, 12, 12), 0.06, seed=r2)
        a, b = IR.per_point(occ, up, r2), IR.layerwise(occ, up, r2)
        assert IR.same(a, b), (up, r2)
        invariants(occ, up, r2, None, b)


@pytest.mark.parametrize("density", [0.3, 0.55, 0.8])
@pytest.mark.parametrize("up", SR.UPS)
def test_regions_against_scipy(up, density):
    ndimage = pytest.importorskip("scipy.ndimage")
    occ = random_occ((9, 14, 11), density, seed=5)
    r = IR.layerwise(occ, up, 1, 0)
    axis = 2 - (SR.up_index(up) >> 1)
    total = 0
    for k in range(occ.shape[axis]):
        layer = np.take(occ, k, axis=axis)
        _, count = ndimage.label(layer)                          # (the default structure: 4-connected)
        h = occ.shape[axis] - 1 - k if SR.up_index(up) & 1 else k
        assert count == r.profile[h, 1]
        labels = np.take(r.labels, k, axis=axis)
        want, _ = ndimage.label(layer)
        # the same partition: each of scipy's components carries one of our numbers, and no number twice
        pairs = set(zip(want[layer != 0].tolist(), labels[layer != 0].tolist()))
        assert len(pairs) == count and len({p[1] for p in pairs}) == count
        total += count
    assert total == r.counts["regions"]


def test_the_empty_and_the_full_lattice():
    for up in SR.UPS:
        r = IR.layerwise(np.zeros(SHAPE, dtype=np.uint8), up, 1)
        assert r.counts == dict.fromkeys(IR.COUNT_NAMES, 0) and not r.mask.any() and not r.labels.any() and not r.profile.any()
        r = IR.layerwise(np.ones(SHAPE, dtype=np.uint8), up, 0)
        nh = SHAPE[2 - (SR.up_index(up) >> 1)]
        assert np.all(r.mask == 1) and r.counts["regions"] == nh and r.counts["islands"] == r.counts["merges"] == 0
        assert IR.roots(r.rows).tolist() == [1] * nh


@pytest.mark.parametrize("form", [IR.per_point, IR.layerwise])
def test_stalactites(form):
    occ = IR.stalactites()
    for r2 in (0, 1, 4):
        r = form(occ, "+z", r2)
        assert r.counts == {"points": 181, "plate": 0, "regions": 18, "base_regions": 1, "islands": 3, "island_points": 3, "merges": 1,
                            "max_layer_regions": 4}
        merges = np.flatnonzero(r.rows[:, IR.BELOW_MIN] != r.rows[:, IR.BELOW_MAX])
        assert len(merges) == 1 and r.rows[merges[0], IR.LAYER] == 8 and r.rows[merges[0], IR.POINTS] == 140       # the slab
        assert r.mask[3, 9, 13] == r.mask[5, 5, 6] == r.mask[7, 5, 10] == 2 and np.count_nonzero(r.mask == 2) == 3
        assert len(set(IR.roots(r.rows).tolist())) == 4
    r = form(occ, "-z", 1)
    assert r.counts == {"points": 181, "plate": 1, "regions": 18, "base_regions": 1, "islands": 0, "island_points": 0, "merges": 0,
                        "max_layer_regions": 4}


def test_sphere():
    occ = IR.sphere24()
    for r2 in (0, 1, 2, 9):
        r = IR.layerwise(occ, "+z", r2, 0)
        assert r.counts == {"points": 2608, "plate": 0, "regions": 18, "base_regions": 0, "islands": 1, "island_points": 4, "merges": 0,
                            "max_layer_regions": 1}
        assert r.rows[0, IR.LAYER] == 3 and r.rows[0, IR.POINTS] == 4
    r = IR.layerwise(occ, "+z", 1)
    assert r.counts["plate"] == 3 and r.counts["islands"] == 0 and r.counts["base_regions"] == 1 and r.counts["regions"] == 18


@pytest.mark.parametrize("form", [IR.per_point, IR.layerwise])
def test_checkerboard(form):
    occ = IR.checkerboard()
    r = form(occ, "+z", 0)
    assert r.counts == {"points": 297, "plate": 0, "regions": 297, "base_regions": 50, "islands": 247, "island_points": 247, "merges": 0,
                        "max_layer_regions": 50}
    assert np.array_equal(r.rows[:, IR.FIRST], np.flatnonzero(occ.reshape(-1)))          # every point its own region, in linear order
    r = form(occ, "+z", 1)
    assert r.counts == {"points": 297, "plate": 0, "regions": 297, "base_regions": 50, "islands": 0, "island_points": 0, "merges": 247,
                        "max_layer_regions": 50}


def test_diagonals_do_not_connect():
    occ = np.zeros((2, 5, 5), dtype=np.uint8)
    occ[:, np.arange(5), np.arange(5)] = 1
    r = IR.layerwise(occ, "+z", 2)
    assert r.counts["regions"] == 10 and r.counts["base_regions"] == 5 and r.counts["merges"] == 5      # each sees itself and a diagonal neighbour below
    assert IR.layerwise(occ, "+z", 1).counts["merges"] == 0


def test_islands_layout_check(tmp_path):
    """tests/cpp/islands_layout_check.cpp under ASan + UBSan: rml::IslandsScratch, rml::IslandsRows, rml::IslTileLds and
    rml::IslLinkLds against offsets written out by hand, the tile and halo indexing of all three frames, and the canonical in-layer
    order against the caller's linear order in all six directions."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    exe = tmp_path / "islands_layout_check"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(root, "include"), "-I", os.path.join(root, "ray-marching_amd", "csrc"), "-o", str(exe),
                            os.path.join(root, "tests", "cpp", "islands_layout_check.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "islands layout ok" in run.stdout


def test_constants_match_the_header():
    import os
    import re
    from ray_marching_amd import _ffi, renderer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rm_abi.h")).read()
    for prefix, names in (("RM_ISL_ROW_", _ffi.ISL_ROW_NAMES), ("RM_ISL_STAT_", _ffi.ISL_STAT_NAMES), ("RM_ISL_", _ffi.ISL_COUNT_NAMES)):
        for k, name in enumerate(names):
            m = re.search(r"\b%s%s = (\d+)" % (prefix, name.upper()), text)
            assert m and int(m.group(1)) == k, (prefix, name)
    assert _ffi.ISL_ROW_NAMES == IR.ROW_NAMES and _ffi.ISL_COUNT_NAMES == IR.COUNT_NAMES
    assert re.search(r"RM_ISL_ROW_WORDS = 12\b", text) and re.search(r"RM_ISL_COUNTS = 8\b", text) and re.search(r"RM_ISL_STATS = 5\b", text)
    assert renderer.ISL_ROW_DTYPE.itemsize == 48 and renderer.ISL_ROW_DTYPE.names == IR.ROW_NAMES


def test_root_loop():
    from ray_marching_amd import renderer
    r = IR.layerwise(IR.stalactites(), "+z", 1)
    rows = np.zeros(len(r.rows), dtype=renderer.ISL_ROW_DTYPE)
    rows.view(np.uint32).reshape(-1, 12)[:] = r.rows
    assert np.array_equal(renderer.island_roots(rows), IR.roots(r.rows)) and np.array_equal(renderer.island_roots(r.rows), IR.roots(r.rows))
    # every region's root is the island or base region that its whole chain of smallest links ends in
    for k, root in enumerate(IR.roots(r.rows)):
        at = k + 1
        while r.rows[at - 1, IR.BELOW_MIN]:
            at = int(r.rows[at - 1, IR.BELOW_MIN])
        assert at == root


def test_printability_gates():
    from ray_marching_amd import islands
    assert islands.parse_gates("islands>0, island_points>12,layer_regions>40") == [("islands", 0.0), ("island_points", 12.0), ("layer_regions", 40.0)]
    assert islands.parse_gates("") == []
    for bad in ("islands", "regions>1", "islands<1", "islands>x", "island_points>"):
        with pytest.raises(ValueError):
            islands.parse_gates(bad)
    values = islands.gate_values({"islands": 3, "island_points": 12, "max_layer_regions": 41})
    assert values == {"islands": 3, "island_points": 12, "layer_regions": 41}
    assert islands.failed_gates(islands.parse_gates("islands>0,island_points>12,layer_regions>41"), values) == ["islands = 3 > 0"]
    assert islands.failed_gates(islands.parse_gates("layer_regions>40"), values) == ["layer_regions = 41 > 40"]


def test_best_direction_tie_breaks():
    from ray_marching_amd import islands

    def reports(**over):
        r = {up: {"islands": 5, "island_points": 70} for up in islands.BEST_ORDER}
        for up, (n, p) in over.items():
            r[{"pz": "+z", "nz": "-z", "py": "+y", "ny": "-y", "px": "+x", "nx": "-x"}[up]] = {"islands": n, "island_points": p}
        return r
    assert islands.BEST_ORDER == ("+z", "-z", "+y", "-y", "+x", "-x")
    assert islands.best_direction(reports()) == "+z"                                # all equal: the order
    assert islands.best_direction(reports(nx=(4, 1000))) == "-x"                    # the fewest islands win over their points
    assert islands.best_direction(reports(ny=(5, 60), px=(5, 60))) == "-y"          # fewer island points, then the order
    assert islands.best_direction(reports(pz=(5, 80), nz=(5, 80))) == "+y"
