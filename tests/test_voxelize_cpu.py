"""Mesh voxelisation without a GPU: the two numpy restatements of the contract agree with each other and with
the exact convex oracle; the result does not depend on triangle order, vertex rotation, reversal or indexing; mesh.read reads what
mesh.write writes (and ASCII STL, ASCII PLY, OBJ with quads and negative indices); the command line's gates; the layouts under
ASan + UBSan as a stand-alone program."""
import os
import struct
import subprocess

import numpy as np
import pytest

import voxel_ref as VR
from ray_marching_amd import mesh, voxelize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
SHAPE = (20, 18, 16)
CENTRE, RADIUS = (9.5, 8.25, 7.75), 6.3

CONVEX = {"ico20": lambda: VR.icosphere(0, RADIUS, CENTRE), "ico80": lambda: VR.icosphere(1, RADIUS, CENTRE),
          "ico320": lambda: VR.icosphere(2, RADIUS, CENTRE), "octahedron": VR.octahedron, "box": lambda: VR.box((3, 2, 4), (12, 11, 9))}
# what the issue's prototype gave: (excluded boundary points, strictly inside points)
PROTOTYPE = {"ico20": (0, 646), "ico80": (0, 914), "ico320": (0, 1018), "octahedron": (146, 231)}


@pytest.mark.parametrize("name", CONVEX)
def test_the_two_restatements_agree_with_each_other_and_the_convex_oracle(name):
    v, t = CONVEX[name]()
    a, ca = VR.voxelize(v, t, *UNIT, SHAPE)
    b, cb = VR.voxelize_by_rows(v, t, *UNIT, SHAPE)
    assert ca == cb and np.array_equal(a, b)
    assert ca["open_rows"] == 0 and ca["rejected"] == 0 and ca["triangles"] == len(t)
    cls = VR.convex_classes(v, t, *UNIT, SHAPE)
    excluded, inside = int((cls == 0).sum()), int((cls == 1).sum())
    if name in PROTOTYPE:
        assert (excluded, inside) == PROTOTYPE[name]
        assert excluded <= 0.03 * cls.size and inside >= 200           # the conditions that keep the comparison honest
    assert np.array_equal(a[cls != 0], (cls[cls != 0] == 1).astype(np.uint8))


def test_the_lattice_aligned_box_is_the_half_open_block():
    v, t = VR.box((3, 2, 4), (12, 11, 9))
    occ, counts = VR.voxelize(v, t, *UNIT, SHAPE)
    want = np.zeros(SHAPE[::-1], np.uint8)
    want[4:9, 3:12, 3:12] = 1
    assert np.array_equal(occ, want) and counts["inside"] == 405 and counts["edge_on"] == 8


def test_torus_keeps_its_hole_and_open_mesh_reports_open_rows():
    v, t = VR.torus()
    occ, counts = VR.voxelize(v, t, *UNIT, (24, 24, 12))
    assert counts["open_rows"] == 0 and counts["inside"] > 500 and occ[:, 10:14, 10:14].sum() == 0
    v, t = VR.icosphere(2, RADIUS, CENTRE)
    a, ca = VR.voxelize(v, t[:-7], *UNIT, SHAPE)
    b, cb = VR.voxelize_by_rows(v, t[:-7], *UNIT, SHAPE)
    assert ca == cb and np.array_equal(a, b) and ca["open_rows"] == 9


def test_invariance_under_order_rotation_reversal_and_indexing():
    v, t = VR.icosphere(1, RADIUS, CENTRE)
    want, cw = VR.voxelize(v, t, *UNIT, SHAPE)
    rng = np.random.default_rng(27)
    variants = {"shuffled": (v, t[rng.permutation(len(t))]), "rotated": (v, np.roll(t, 1, axis=1)), "reversed": (v, t[:, ::-1]),
                "soup": (VR.soup_of(v, t), None)}
    for name, (vv, tt) in variants.items():
        for f in (VR.voxelize, VR.voxelize_by_rows):
            occ, counts = f(vv, tt, *UNIT, SHAPE)
            assert np.array_equal(occ, want) and counts == cw, name


def test_snapping_and_rejection():
    q, ok = VR.snap([[0.1, 1.0 / 3.0, 2048.0], [np.nan, np.inf, 2048.5]], (0, 0, 0), (1, 1, 1))
    assert q[0].tolist() == [6, 21, 131072] and ok.tolist() == [[True, True, True], [False, False, False]]
    assert VR.snap([[0.0078125, 0.0234375, -0.0078125]], (0, 0, 0), (1, 1, 1))[0][0].tolist() == [0, 2, 0]     # halves to even
    v, t = VR.icosphere(0, RADIUS, CENTRE)
    want, cw = VR.voxelize(v, t, *UNIT, SHAPE)
    vv = np.concatenate([v, [[np.nan, 1, 1], [1, 1, 1], [2, 5, 1], [3000, 1, 1]]]).astype(np.float32)
    n = len(v)
    tt = np.concatenate([t, [[n, n + 1, n + 2], [n + 1, n + 2, n + 3], [0, 1, n + 4]]]).astype(np.uint32)
    occ, counts = VR.voxelize(vv, tt, *UNIT, SHAPE)
    assert counts["rejected"] == 3 and counts["triangles"] == len(t) + 3
    assert np.array_equal(occ, want) and all(counts[k] == cw[k] for k in ("edge_on", "crossings", "inside", "open_rows"))


def quad_mesh():
    v, t = VR.box((0.5, 0.25, 0.125), (3.5, 2.25, 1.125))
    return mesh.Mesh(v, t)


@pytest.mark.parametrize("ext", ["obj", "ply", "stl"])
def test_read_reads_what_write_writes(tmp_path, ext):
    m = mesh.Mesh(*VR.icosphere(1, 1.7, (0.3, -0.2, 0.1)))
    path = str(tmp_path / ("m." + ext))
    mesh.write(m, path)
    r = mesh.read(path)
    if ext == "stl":                                                           # a soup in file order
        assert np.array_equal(r.vertices, VR.soup_of(m.vertices, m.triangles))
        assert np.array_equal(r.triangles, np.arange(3 * len(m.triangles), dtype=np.uint32).reshape(-1, 3))
    else:
        assert r.vertices.dtype == np.float32 and np.array_equal(r.vertices, m.vertices)     # %.9g round-trips float32
        assert r.triangles.dtype == np.uint32 and np.array_equal(r.triangles, m.triangles)
    a, ca = VR.voxelize(r.vertices, r.triangles, (-2, -2, -2), (0.25, 0.25, 0.25), (17, 17, 17))
    b, cb = VR.voxelize(m.vertices, m.triangles, (-2, -2, -2), (0.25, 0.25, 0.25), (17, 17, 17))
    assert np.array_equal(a, b) and ca == cb


def test_read_ascii_stl_ascii_ply_and_obj_with_quads(tmp_path):
    m = quad_mesh()
    soup = VR.soup_of(m.vertices, m.triangles)
    p = tmp_path / "a.stl"
    with open(p, "w") as f:
        f.write("solid part\n")
        for k in range(0, len(soup), 3):
            f.write(" facet normal 0 0 0\n  outer loop\n")
            f.writelines("   vertex %.9g %.9g %.9g\n" % tuple(x) for x in soup[k:k + 3].tolist())
            f.write("  endloop\n endfacet\n")
        f.write("endsolid part\n")
    r = mesh.read(str(p))
    assert np.array_equal(r.vertices, soup) and len(r.triangles) == 12
    # a binary STL whose header begins with "solid"
    p = tmp_path / "b.stl"
    with open(p, "wb") as f:
        f.write(b"solid but binary".ljust(80, b" ") + struct.pack("<I", 1) + struct.pack("<12fH", 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0))
    assert mesh.read(str(p)).vertices.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    p = tmp_path / "a.ply"
    with open(p, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 8\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nelement face 6\nproperty list uchar int vertex_indices\nend_header\n")
        f.writelines("%.9g %.9g %.9g 255\n" % tuple(x) for x in m.vertices.tolist())
        quads = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (0, 4, 7, 3)]
        f.writelines("4 %d %d %d %d\n" % q for q in quads)
    r = mesh.read(str(p))
    assert np.array_equal(r.vertices, m.vertices) and np.array_equal(r.triangles, m.triangles)          # fanned as VR.box splits
    p = tmp_path / "q.obj"
    with open(p, "w") as f:
        f.write("# quads, a texture index, negative indices\n")
        f.writelines("v %.9g %.9g %.9g\n" % tuple(x) for x in m.vertices.tolist())
        f.write("vt 0 0\n")
        for q in quads[:5]:
            f.write("f " + " ".join("%d/1" % (k + 1) for k in q) + "\n")
        f.write("f " + " ".join("%d" % (k - 8) for k in quads[5]) + "\n")
    r = mesh.read(str(p))
    assert np.array_equal(r.vertices, m.vertices) and np.array_equal(r.triangles, m.triangles)
    with pytest.raises(ValueError):
        mesh.read(str(tmp_path / "part.step"))


def test_gate_parsing():
    assert voxelize.parse_reports("topology, thickness") == ["topology", "thickness"] and voxelize.parse_reports("") == []
    with pytest.raises(ValueError):
        voxelize.parse_reports("topology,volume")
    g = voxelize.parse_gates("open_rows>0, rejected>0,bodies>1,inscribed_radius<0.4,topology.points>1e6", ["topology", "thickness"])
    assert g == [("open_rows", ">", 0.0), ("rejected", ">", 0.0), ("bodies", ">", 1.0), ("inscribed_radius", "<", 0.4), ("topology.points", ">", 1e6)]
    assert voxelize.parse_gates("") == []
    for bad in ("open_rows", "bodies>1", "open_rows>x", "open_rows=0", "islands>0"):      # (bodies: no topology report requested)
        with pytest.raises(ValueError):
            voxelize.parse_gates(bad, [])
    report = {"voxels": {"open_rows": 3, "rejected": 0}, "topology": {"bodies": 2, "points": 10}, "thickness": {"points": 11, "inscribed_radius": 0.5}}
    values = voxelize.gate_values(report, ["topology", "thickness"])
    assert values["points"] == 10 and values["thickness.points"] == 11
    failed = voxelize.failed_gates(g, values)
    assert failed == ["open_rows = 3 > 0", "bodies = 2 > 1"]


def test_voxel_layout_check(tmp_path):
    """tests/cpp/voxel_layout_check.cpp under ASan + UBSan: rml::VoxScratch and rml::VoxFillLds against offsets written out by hand,
    and the fill kernel's indexing restated on the host."""
    cxx = os.environ.get("CXX", "g++")
    exe = tmp_path / "voxel_layout_check"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"), "-o", str(exe),
                            os.path.join(ROOT, "tests", "cpp", "voxel_layout_check.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "voxel layout ok" in run.stdout
