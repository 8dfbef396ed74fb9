"""Lattice meshing without a GPU: the contract's restatement tests/class_mesh_ref.py against a second,
per-face restatement in plain loops, its known answers, and its identities with the other contracts' restatements -- the face
counts are surface_ref's PAIR sums, the triangle areas its FACET_AREA, the mesh is closed when B is the complement of A, it
voxelises back to the lattice it came from (voxel_ref), and its Euler number is the shape's.  Then the layouts and the bindings."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import class_mesh_ref as CR
import lattice_cases
import surface_ref as SR
import voxel_ref
from ray_marching_amd import _ffi, mesh, renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLID = [1, 2, 3, 4, 5, 6, 7]


def random_classes(seed, shape=(5, 4, 6), top=10):
    return np.random.default_rng(seed).integers(0, top, size=shape, dtype=np.uint8)


# ---- a second restatement: one face at a time ---------------------------------------------------------------------------------------
def brute(data, set_a, set_b, origin, step):
    c = CR.classes_of(data)
    nz, ny, nx = c.shape
    cx, cy = nx + 1, ny + 1

    def cls(i, j, k):
        return int(c[k, j, i]) if 0 <= i < nx and 0 <= j < ny and 0 <= k < nz else 0

    faces = {}
    for k in range(-1, nz + 1):
        for j in range(-1, ny + 1):
            for i in range(-1, nx + 1):
                for a in range(3):
                    p, q = [i, j, k], [i, j, k]
                    q[a] += 1
                    if q[a] > (nx, ny, nz)[a]:
                        continue
                    cp, cq = cls(*p), cls(*q)
                    if cp in set_a and cq in set_b:
                        side, other, positive = p, cq, 1
                    elif cp in set_b and cq in set_a:
                        side, other, positive = q, cp, 0
                    else:
                        continue
                    L = q[0] + cx * (q[1] + cy * q[2])
                    inside = 0 <= side[0] < nx and 0 <= side[1] < ny and 0 <= side[2] < nz
                    faces[3 * L + a] = (q, a, positive, cls(*side) | other << 8 | (2 * a + positive) << 16,
                                        side[0] + nx * (side[1] + ny * side[2]) if inside else CR.NO_ID)
    quads, corners, edges = [], set(), {}
    for key in sorted(faces):
        q, a, positive, word0, word1 = faces[key]
        u, v = (a + 1) % 3, (a + 2) % 3
        quad = []
        for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
            r = list(q)
            r[u] += du
            r[v] += dv
            quad.append(r[0] + cx * (r[1] + cy * r[2]))
        corners.update(quad)
        for lower, direction in ((quad[0], u), (quad[0], v), (quad[3], u), (quad[1], v)):
            edges[(lower, direction)] = edges.get((lower, direction), 0) + 1
        quads.append((quad, positive, word0, word1))
    order = sorted(corners)
    rank = {L: n for n, L in enumerate(order)}
    o, s = np.asarray(origin, dtype=np.float32), np.asarray(step, dtype=np.float32)
    vertices = np.zeros((len(order), 3), dtype=np.float32)
    for n, L in enumerate(order):
        for axis, coordinate in enumerate((L % cx, (L // cx) % cy, L // (cx * cy))):
            vertices[n, axis] = o[axis] + np.float32((np.float32(coordinate) - np.float32(0.5)) * s[axis])
    triangles, ids = [], []
    for quad, positive, word0, word1 in quads:
        q00, q10, q11, q01 = (rank[L] for L in quad)
        triangles += [(q00, q10, q11), (q00, q11, q01)] if positive else [(q00, q11, q10), (q00, q01, q11)]
        ids += [(word0, word1)] * 2
    n = list(edges.values())
    counts = {"vertices": len(order), "triangles": 2 * len(quads), "faces": len(quads), "edges": len(n),
              "open_edges": sum(1 for x in n if x in (1, 3)), "branch_edges": sum(1 for x in n if x >= 3)}
    for a, name in enumerate("xyz"):
        counts["faces_pos_" + name] = sum(1 for f in faces.values() if f[1] == a and f[2])
        counts["faces_neg_" + name] = sum(1 for f in faces.values() if f[1] == a and not f[2])
    return {"vertices": vertices, "triangles": np.array(triangles, dtype=np.uint32).reshape(-1, 3),
            "ids": np.array(ids, dtype=np.uint32).reshape(-1, 2), "counts": counts}


@pytest.mark.parametrize("sets", [(SOLID, [0]), ([0], SOLID), ([1, 2], [3, 7]), ([7], [0, 1])])
@pytest.mark.parametrize("seed", range(3))
def test_restatement_equals_the_per_face_one(seed, sets):
    data = random_classes(seed, shape=[(5, 4, 6), (2, 2, 2), (3, 7, 2)][seed])
    origin, step = (-1.25, 0.5, 2.0), (0.25, 0.5, 0.375)
    got, ref = CR.mesh(data, *sets, origin, step), brute(data, *sets, origin, step)
    assert got["counts"] == ref["counts"]
    for name in ("vertices", "triangles", "ids"):
        assert got[name].dtype == ref[name].dtype and np.array_equal(got[name].view(np.uint32), ref[name].view(np.uint32)), name


# ---- known answers --------------------------------------------------------------------------------------------------------------------
def test_one_voxel_in_a_corner():
    data = np.zeros((2, 2, 2), dtype=np.uint8)
    data[0, 0, 0] = 1
    m = CR.mesh(data, SOLID, [0])
    assert m["counts"]["vertices"] == 8 and m["counts"]["triangles"] == 12 and m["counts"]["edges"] == 12
    assert tuple(m["triangles"][0]) == (0, 6, 2) and tuple(m["vertices"][0]) == (-0.5, -0.5, -0.5)
    assert tuple(m["ids"][0]) == (1, 0)
    assert [m["counts"]["faces_%s_%s" % (s, a)] for a in "xyz" for s in ("pos", "neg")] == [1] * 6


def test_full_two_cubed():
    c = CR.mesh(np.ones((2, 2, 2), dtype=np.uint8), SOLID, [0])["counts"]
    assert (c["vertices"], c["triangles"], c["edges"], c["open_edges"], c["branch_edges"]) == (26, 48, 48, 0, 0)


def test_empty_mesh():
    m = CR.mesh(np.zeros((3, 2, 4), dtype=np.uint8), SOLID, [0])
    assert m["vertices"].shape == (0, 3) and m["triangles"].shape == (0, 3) and m["ids"].shape == (0, 2)
    assert all(v == 0 for v in m["counts"].values())


# ---- identities -----------------------------------------------------------------------------------------------------------------------
def identity_lattices():
    shape = (19, 17, 18)
    for kind in lattice_cases.CONTENTS:
        yield kind, lattice_cases.contents(shape, kind, seed=7)
    yield "checkerboard", CR.checkerboard((6, 5, 7))


def as_mesh(m):
    return mesh.Mesh(m["vertices"], m["triangles"])


def triangle_area(m):
    p = m["vertices"].astype(np.float64)[m["triangles"].astype(np.int64)]
    return 0.5 * float(np.sqrt((np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]) ** 2).sum(axis=1)).sum())


@pytest.mark.parametrize("name,data", list(identity_lattices()), ids=[n for n, _ in identity_lattices()])
def test_face_counts_areas_and_closure(name, data):
    # A vertex coordinate o + (c - 0.5) s is exact in binary32 when o and s are small dyadic numbers (c - 0.5 has at most 11
    # significant bits, the lattices here have c <= 20); then every triangle is half a rectangle with exactly representable sides
    # and the bound on |sum of areas - FACET_AREA| from the vertex rounding is 0.  (In general it is 4 ulp(|o| + n s) per side.)
    origin, step = (-1.25, 0.5, 2.0), (0.25, 0.5, 0.375)
    words = SR.counts(data)
    P = SR.pairs(words)
    for A, B in ((SOLID, [0]), ([0], SOLID), ([1, 3], [0, 7]), ([3], [0])):
        m = CR.mesh(data, A, B, origin, step)
        for ax, axis_name in enumerate("xyz"):
            assert m["counts"]["faces_pos_" + axis_name] == sum(int(P[a, b, ax]) for a in A for b in B)
            assert m["counts"]["faces_neg_" + axis_name] == sum(int(P[b, a, ax]) for a in A for b in B)
        assert triangle_area(m) == SR.measures(words, step, A, B)["facet_area"]
        present = set(np.unique(CR.classes_of(data)).tolist()) | {0}
        if present <= set(A) | set(B):
            assert as_mesh(m).is_closed() and m["counts"]["open_edges"] == 0
        else:                                                   # (a border only where a class left out touches A)
            assert as_mesh(m).is_closed() == (m["counts"]["open_edges"] == 0)


def test_a_pair_that_leaves_a_class_out_has_a_border():
    data = np.zeros((4, 4, 4), dtype=np.uint8)
    data[1:3, 1:3, 1] = 1
    data[1:3, 1:3, 2] = 2                                       # class 2 on top of class 1
    m = CR.mesh(data, [1], [0])
    assert m["counts"]["open_edges"] == 8 and not as_mesh(m).is_closed()
    assert CR.mesh(data, [1], [0, 2])["counts"]["open_edges"] == 0


@pytest.mark.parametrize("name,data", list(identity_lattices()), ids=[n for n, _ in identity_lattices()])
def test_round_trip_through_the_voxeliser(name, data):
    origin, step = (-1.25, 0.5, 2.0), (0.25, 0.5, 0.375)
    m = CR.mesh(data, SOLID, [0], origin, step)
    if m["counts"]["faces"] == 0:
        return
    nz, ny, nx = data.shape
    occ, counts = voxel_ref.voxelize(m["vertices"], m["triangles"], origin, step, (nx, ny, nz))
    assert np.array_equal(occ != 0, data != 0) and counts["open_rows"] == 0 and counts["rejected"] == 0


def test_euler_number():
    for data, euler in ((SR.ball(7.3, (0.2, 0.1, 0.4)), 2), (CR.torus(9.0, 3.4), 0)):
        c = CR.mesh(data, [1], [0])["counts"]
        assert c["branch_edges"] == 0 and c["open_edges"] == 0
        assert c["vertices"] - c["edges"] + c["faces"] == euler
    assert CR.mesh(CR.checkerboard((4, 4, 4)), [1], [0])["counts"]["branch_edges"] > 0


# ---- layout ---------------------------------------------------------------------------------------------------------------------------
def test_class_mesh_layout_check(tmp_path):
    """tests/cpp/class_mesh_layout_check.cpp under ASan + UBSan: rml::ClassMeshScratch and rml::ClassMeshSlot against offsets
    written out by hand, and a walk over the words as the kernels index them."""
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    exe = tmp_path / "class_mesh_layout_check"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"), "-o", str(exe),
                            os.path.join(ROOT, "tests", "cpp", "class_mesh_layout_check.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "class mesh layout ok" in run.stdout


# ---- bindings -------------------------------------------------------------------------------------------------------------------------
def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "rm_abi.h")).read()
    for k, name in enumerate(_ffi.CMESH_COUNT_NAMES):
        m = re.search(r"\bRM_CMESH_%s = (\d+)" % name.upper(), text)
        assert m and int(m.group(1)) == k == getattr(_ffi, "RM_CMESH_" + name.upper()), name
    for k, name in enumerate(_ffi.CMESH_STAT_NAMES):
        m = re.search(r"\bRM_CMESH_STAT_%s = (\d+)" % name.upper(), text)
        assert m and int(m.group(1)) == k == getattr(_ffi, "RM_CMESH_STAT_" + name.upper()), name
    assert re.search(r"\bRM_CMESH_COUNTS = 12\b", text) and _ffi.RM_CMESH_COUNTS == 12 == len(CR.COUNT_NAMES)
    assert re.search(r"\bRM_CMESH_STATS = 6\b", text) and _ffi.RM_CMESH_STATS == 6
    assert _ffi.CMESH_COUNT_NAMES == CR.COUNT_NAMES and _ffi.RM_NO_ID == CR.NO_ID


def test_rust_wrappers_are_present():
    text = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in ("fn rm_mesh_classes(", "fn rm_read_class_mesh(", "pub fn mesh_classes(", "pub fn read_class_mesh(", "pub const RM_CMESH_COUNTS: c_int = 12;",
                 "pub const RM_CMESH_BRANCH_EDGES: c_int = 11;", "pub const RM_CMESH_STATS: c_int = 6;", "pub struct ClassMesh"):
        assert name in text, name


class _NoLibrary:
    """Stands in for the library: any call is an error."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


@pytest.mark.parametrize("a,b", [([], None), ([1], [1, 2]), ([8], None), ([1], []), (list(range(8)), None), (-1, [0])])
def test_python_refuses_bad_masks_before_any_library_call(a, b):
    r = object.__new__(renderer.RayMarchingResources)
    r._L, r._h = _NoLibrary(), None
    with pytest.raises(ValueError):
        r.mesh_classes(np.zeros((2, 2, 2), dtype=np.uint8), a, b)
