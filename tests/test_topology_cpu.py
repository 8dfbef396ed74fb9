"""The yardstick of the solid-topology tests (tests/topology_ref.py), checked without a GPU: against
scipy.ndimage.label where scipy is installed, and on hand-built occupancies whose bodies, cavities, Euler characteristic and
tunnels are known."""
import numpy as np
import pytest

import mass_ref as M
import topology_cases as TC
import topology_ref as TR

F = np.float32


def empty(nz, ny, nx):
    return np.zeros((nz, ny, nx), dtype=bool)


def summary(t):
    c = t["counts"]
    return c["bodies"], c["cavities"], c["euler"], c["tunnels"]


def same_partition(a, b):
    """Two labelings of the same points induce the same partition: the pairs (a, b) are in one-to-one correspondence."""
    pairs = np.unique(np.stack([np.asarray(a).ravel(), np.asarray(b).ravel()]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))


def consistent(t, inside):
    """What holds for every result: the label classes, the numbering, the rows against the labels, and the sums."""
    lab, c = t["labels"], t["counts"]
    assert lab.dtype == np.uint32 and lab.shape == inside.shape
    assert np.array_equal(lab < TR.CAVITY_BIT, inside)
    assert c["points"] == np.count_nonzero(inside)
    assert c["exterior_points"] == np.count_nonzero(lab == TR.EXTERIOR)
    assert c["tunnels"] == c["bodies"] + c["cavities"] - c["euler"]
    kk, jj, ii = np.meshgrid(*(np.arange(n) for n in inside.shape), indexing="ij")
    first = -1
    for b, row in enumerate(t["body_rows"]):
        sel = lab == b
        assert row == M.moments_of_indices(ii[sel], jj[sel], kk[sel])
        lowest = int(np.flatnonzero(sel.ravel())[0])
        assert lowest > first                                               # numbered by smallest linear index
        first = lowest
    first = -1
    for q, row in enumerate(t["cavity_rows"]):
        sel = lab == (TR.CAVITY_BIT | q)
        assert row == M.moments_of_indices(ii[sel], jj[sel], kk[sel])
        lowest = int(np.flatnonzero(sel.ravel())[0])
        assert lowest > first
        first = lowest
    assert TR.combine_rows(t["body_rows"]) == M.moments_of_inside(inside)
    total = c["points"] + c["exterior_points"] + sum(r[0] for r in t["cavity_rows"])
    assert total == inside.size


# ---- hand-built occupancies -----------------------------------------------------------------------------------------------------
def test_cubes_sharing_only_an_edge_are_two_bodies_and_the_gap_joins_the_voids():
    a = empty(6, 6, 6)
    a[1:3, 1:3, 1:3] = True
    a[1:3, 3:5, 3:5] = True                                                 # share the edge j = 2|3, i = 2|3
    t = TR.topology(a)
    consistent(t, a)
    assert summary(t)[:2] == (2, 0)
    # the two voids on either side of the shared edge, (j, i) = (2, 3) and (3, 2), are one void: fill everything else
    b = np.ones((4, 6, 6), dtype=bool)
    b[1:3, 2, 3] = False
    b[1:3, 3, 2] = False
    t = TR.topology(b)
    consistent(t, b)
    assert t["counts"]["cavities"] == 1 and t["cavity_rows"][0][0] == 4


def test_cubes_sharing_only_a_corner_are_two_bodies():
    a = empty(6, 6, 6)
    a[1:3, 1:3, 1:3] = True
    a[3:5, 3:5, 3:5] = True
    t = TR.topology(a)
    consistent(t, a)
    assert summary(t) == (2, 0, 2, 0)
    b = np.ones((4, 4, 4), dtype=bool)                                      # two buried outside points that touch at a corner
    b[1, 1, 1] = False
    b[2, 2, 2] = False
    t = TR.topology(b)
    consistent(t, b)
    assert t["counts"]["cavities"] == 1 and t["cavity_rows"][0][0] == 2


def test_shell_has_one_cavity():
    a = empty(5, 5, 5)
    a[1:4, 1:4, 1:4] = True
    a[2, 2, 2] = False
    t = TR.topology(a)
    consistent(t, a)
    assert summary(t) == (1, 1, 2, 0)
    assert t["labels"][2, 2, 2] == TR.CAVITY_BIT and t["cavity_rows"][0][:4] == [1, 2, 2, 2]


def test_voxel_ring_has_one_tunnel():
    a = empty(3, 5, 5)
    a[1, 1:4, 1:4] = True
    a[1, 2, 2] = False
    t = TR.topology(a)
    consistent(t, a)
    assert summary(t) == (1, 0, 0, 1)


def test_void_reaching_the_border_through_a_diagonal_gap_is_exterior():
    a = np.ones((5, 5, 5), dtype=bool)
    a[2, 2, 2] = False
    closed = TR.topology(a)
    assert closed["counts"]["cavities"] == 1
    a[1, 1, 1] = False
    a[0, 0, 0] = False                                                       # a chain of corner contacts to the border
    t = TR.topology(a)
    consistent(t, a)
    assert t["counts"]["cavities"] == 0 and t["counts"]["exterior_points"] == 3
    assert t["counts"]["bodies"] == 1


def test_full_and_empty():
    t = TR.topology(np.ones((2, 3, 4), dtype=bool))
    assert summary(t) == (1, 0, 1, 0) and t["counts"]["exterior_points"] == 0
    t = TR.topology(empty(2, 3, 4))
    assert summary(t) == (0, 0, 0, 0) and t["counts"]["exterior_points"] == 24 and np.all(t["labels"] == TR.EXTERIOR)


# ---- the hand-built cases of the GPU tests (tests/topology_cases.py): their literals against the restatement ---------------------
def test_border_case_generator_counts():
    assert len(TC.OFFSETS) == 26 and len(TC.BORDER_CASES) == 124 == 6 * 2 + 12 * 4 + 8 * 8
    assert len(set(TC.BORDER_CASES)) == 124
    for d, s in TC.BORDER_CASES:
        a, b = TC.pair(d, s)
        assert tuple(y - x for x, y in zip(a, b)) == d
        for x in range(3):
            assert (a[x] // 8 != b[x] // 8) == (x in s)                         # a border exactly on the axes in s
            assert x in s or d[x] == 0 or 1 <= min(a[x], b[x]) % 8 and max(a[x], b[x]) % 8 <= 6   # well inside one brick otherwise


@pytest.mark.parametrize("inside", [True, False])
@pytest.mark.parametrize("d", TC.OFFSETS)
def test_border_pairs_literals_against_the_restatement(d, inside):
    pairs = TC.packed_pairs(d)
    assert len(pairs) == 2 ** TC.faces_of(d)
    occ = TC.occupancy_of(pairs, TC.PACKED_SHAPE, inside)
    t = TR.topology(occ)
    TC.check_expected(t["counts"], t["cavity_rows"], TC.expected_of_pairs(d, pairs, TC.PACKED_SHAPE, inside))
    if not inside:
        assert t["counts"]["exterior_points"] == 0 and t["counts"]["cavities"] == len(pairs)
    # thin last bricks: i = 16 is the lattice's border there
    pairs = [TC.thin_pair(d)]
    occ = TC.occupancy_of(pairs, TC.THIN_SHAPE, inside)
    t = TR.topology(occ)
    want = TC.expected_of_pairs(d, pairs, TC.THIN_SHAPE, inside)
    TC.check_expected(t["counts"], t["cavity_rows"], want)
    if not inside:
        assert (want["cavities"], want["exterior_points"]) == ((0, 2) if d[0] != 0 else (1, 0))


@pytest.mark.parametrize("way", sorted(TC.SNAKE_WAYS))
def test_snake_literals_against_the_restatement(way):
    for mirror in TC.ORIENTATIONS:
        occ = TC.snake_case(way, mirror)
        t = TR.topology(occ)
        assert summary(t) == TC.SNAKE_WAYS[way], mirror
        if way == "complement":
            assert t["cavity_rows"][0][0] == TC.SNAKE_POINTS == 143
        else:
            assert t["counts"]["points"] == TC.SNAKE_POINTS and t["counts"]["edges"] == TC.SNAKE_POINTS - 1   # a path


def test_checkerboard_frames_and_rods_literals_against_the_restatement():
    t = TR.topology(TC.checkerboard(TC.SMALL))
    assert summary(t) == (5610, 0, 5610, 0) and t["counts"]["exterior_points"] == 5610
    t = TR.topology(TC.checkerboard(TC.SMALL, 1))
    assert summary(t) == (5610, 0, 5610, 0) and t["counts"]["exterior_points"] == 5610
    for axis, want in TC.FRAMED.items():
        assert summary(TR.topology(TC.framed_planes(axis))) == want, axis
    t = TR.topology(TC.rods())
    assert summary(t) == (90, 0, 90, 0) and all(r[0] == 33 for r in t["body_rows"])
    t = TR.topology(TC.buried_voids(8))                                       # the small sibling of the 64^3 case
    assert summary(t)[:2] == (1, 27) and all(r[0] == 1 for r in t["cavity_rows"])


# ---- random occupancies ---------------------------------------------------------------------------------------------------------
def random_occupancy(seed, density, shape=(17, 20, 33)):
    return np.random.default_rng(seed).random(shape) < density


@pytest.mark.parametrize("density", [0.2, 0.3116, 0.5, 0.9])
def test_random_occupancies_are_consistent(density):
    a = random_occupancy(5, density)
    t = TR.topology(a)
    consistent(t, a)


@pytest.mark.parametrize("seed,density", [(s, d) for s in (5, 6) for d in (0.2, 0.3116, 0.5, 0.9)])
def test_reference_agrees_with_scipy(seed, density):
    ndi = pytest.importorskip("scipy.ndimage")
    a = random_occupancy(seed, density)
    t = TR.topology(a)
    lab6, n6 = ndi.label(a, structure=ndi.generate_binary_structure(3, 1))
    assert t["counts"]["bodies"] == n6
    assert same_partition(t["labels"][a], lab6[a])
    outside_p = np.pad(~a, 1, constant_values=True)
    lab26, n26 = ndi.label(outside_p, structure=ndi.generate_binary_structure(3, 3))
    assert t["counts"]["cavities"] == n26 - 1
    exterior = (lab26 == lab26[0, 0, 0])[1:-1, 1:-1, 1:-1] & ~a
    assert np.array_equal(t["labels"] == TR.EXTERIOR, exterior)
    cav = ~a & ~exterior
    assert same_partition(t["labels"][cav], lab26[1:-1, 1:-1, 1:-1][cav])


# ---- the interface, as far as it goes without a GPU ---------------------------------------------------------------------------------
def test_constants_match_the_header_and_the_symbols_are_exported():
    import os
    import re
    from ray_marching_amd import _ffi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rm_abi.h")).read()
    for enum in ("rm_topocount", "rm_topostat"):
        body = re.search(r"enum\s+%s\s*\{(.*?)\}" % enum, text, re.S).group(1)
        pairs = re.findall(r"(RM_[A-Z0-9_]+)\s*=\s*(\d+)", body)
        assert len(pairs) >= 7
        for name, value in pairs:
            assert getattr(_ffi, name) == int(value), name
    assert len(_ffi.TOPO_COUNT_NAMES) == _ffi.RM_TOPO_COUNTS and TR.COUNT_NAMES == _ffi.TOPO_COUNT_NAMES
    assert len(_ffi.TOPO_STAT_NAMES) == _ffi.RM_TOPO_STATS
    assert int(re.search(r"#define RM_TOPO_CAVITY_BIT (0x[0-9A-Fa-f]+)u", text).group(1), 16) == _ffi.RM_TOPO_CAVITY_BIT == TR.CAVITY_BIT
    assert int(re.search(r"#define RM_TOPO_EXTERIOR (0x[0-9A-Fa-f]+)u", text).group(1), 16) == _ffi.RM_TOPO_EXTERIOR == TR.EXTERIOR
    L = _ffi.hip_lib()
    for fn in ("rm_label_solid", "rm_label_occupancy", "rm_read_topology"):
        assert hasattr(L, fn)
    assert L.rm_abi_version() == 2
    counts, stats = (np.zeros(n, dtype=np.uint64) for n in (_ffi.RM_TOPO_COUNTS, _ffi.RM_TOPO_STATS))
    assert L.rm_read_topology(None, None, None, None, 0, None) == _ffi.RM_ERR_NULL
    assert L.rm_label_occupancy(None, 2, 2, 2, counts.ctypes.data, 0, None, counts.ctypes.data_as(_ffi.C.POINTER(_ffi.C.c_uint64)),
                                _ffi.RM_TOPO_COUNTS, stats.ctypes.data_as(_ffi.C.POINTER(_ffi.C.c_uint64)), _ffi.RM_TOPO_STATS) == _ffi.RM_ERR_NULL


def test_scratch_and_result_layouts(tmp_path):
    """tests/cpp/topology_layout_check.cpp under ASan + UBSan: rml::TopoScratch and rml::TopoRows against offsets written out by hand."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    exe = tmp_path / "topology_layout_check"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(root, "include"), "-I", os.path.join(root, "ray-marching_amd", "csrc"), "-o", str(exe),
                            os.path.join(root, "tests", "cpp", "topology_layout_check.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "topology layout ok" in run.stdout


def test_printability_gates():
    from ray_marching_amd import topology
    assert topology.parse_gates("bodies>1, cavities>0") == [("bodies", 1), ("cavities", 0)]
    assert topology.parse_gates("") == []
    for bad in ("bodies", "volume>1", "bodies<1", "bodies>x"):
        with pytest.raises(ValueError):
            topology.parse_gates(bad)
    counts = {"bodies": 13, "cavities": 0, "tunnels": 0}
    assert topology.failed_gates(topology.parse_gates("bodies>1,cavities>0"), counts) == ["bodies = 13 > 1"]
    assert topology.failed_gates(topology.parse_gates("bodies>13"), counts) == []


def test_body_rows_sum_to_the_lattice_moments_of_a_scene(oracle):
    import test_sparse_mesh_cpu as T
    cc, w = oracle.serialize(*T.ALL_SCENES["g8"]())
    origin, step, shape = (-2.5,) * 3, (F(5.0) / F(23),) * 3, (24, 24, 24)
    t = TR.solid(cc, w, origin, step, shape, 0.0)
    inside = M.lattice_inside(cc, w, origin, step, shape, 0.0)
    consistent(t, inside)
    assert TR.combine_rows(t["body_rows"]) == M.lattice_moments(cc, w, origin, step, shape, 0.0)
    assert t["counts"]["bodies"] >= 1
