"""Mesh slicing on the GPU (rm_slice_mesh, read with rm_read_slices): counts, points bit for bit, contours and
layer_first == the numpy restatement (tests/mesh_slice_ref.py) for its known-answer meshes on all three axes, a level-5 icosphere in
300 layers (several sort tiles, more than one ranking block, chains longer than 256), rejected triangles, one layer and layers that
miss the mesh, device inputs and a device read, two runs, the invariances, isolation from the other retained results, every refusal
with the previous slices still readable, and the round trip extract_mesh -> weld -> slice_mesh against slice_contours."""
import ctypes as C

import numpy as np
import pytest

import mesh_slice_ref as R
import voxel_ref as VR
from ray_marching_amd import _ffi, csg, mesh, renderer, slicer

pytestmark = pytest.mark.gpu

O, S = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
CASES = R.cases()
# The round trip's margin on a layer's area, relative to the area.  Both outlines are polygons on the circle of radius r >= 0.6 in
# which the plane cuts g1's unit sphere: their chords span at most theta = sqrt(3) step / r (a cell's diagonal), which costs an
# inscribed polygon at most theta^2 / 6 = 2.1e-3 of the disc, and linear interpolation along a lattice edge misplaces a vertex by at
# most step^2 / (8 r) radially, step^2 / (4 r^2) = 1.1e-3 of the area: 3.2e-3 in all, step = 5 / 128.  Measured with the CPU
# restatements (mesh_ref -> weld -> mesh_slice_ref against slice_ref, the same planes): at most 1.14e-3.  
ROUND_TRIP_MARGIN = 3.2e-3


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)      # no program: slicing a mesh needs none
    yield r
    r.close()


def same(got, want, what=""):
    g = got.numpy()
    print("%s: counts %s; stats %s" % (what, got.counts, got.stats))
    assert got.counts == want["counts"], what
    assert g.points.dtype == np.float32 and g.points.shape == want["points"].shape, what
    assert np.array_equal(g.points.view(np.uint32), want["points"].view(np.uint32)), what
    assert np.array_equal(g.contours, want["contours"]) and np.array_equal(g.layer_first, want["layer_first"]), what
    assert got.lattice is None and got.stats["scratch_bytes"] > 0


def as_result(s):
    g = s.numpy()
    return {"points": g.points, "contours": g.contours, "layer_first": g.layer_first, "counts": s.counts}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("w", range(3))
def test_known_answer_meshes(res, name, w):
    v, t, h = CASES[name]
    same(res.slice_mesh(v, t, O, S, w, heights=h), R.slice_mesh(v, t, O, S, w, h), "%s %d" % (name, w))


def test_awkward_frame(res):
    v, t = VR.icosphere(2, 3.3, (0.4, -0.7, 1.9))
    o, s, h = (-4.25, -5.5, -2.125), (0.0625, 0.07, 0.11), np.arange(-1.3, 5.2, 0.173)
    for w in range(3):
        same(res.slice_mesh(v, t, o, s, w, heights=h), R.slice_mesh(v, t, o, s, w, h), "awkward %d" % w)


@pytest.fixture(scope="module")
def big():
    v, t = VR.icosphere(5, 100.0, (120.3, 119.2, 121.1))
    h = 21.7 + np.arange(300) * 0.66
    return v, t, h, R.slice_mesh(v, t, O, S, 2, h)


def test_level_5_icosphere_in_300_layers(res, big):
    v, t, h, want = big
    got = res.slice_mesh(v, t, O, S, 2, heights=h)
    same(got, want, "icosphere 5")
    assert got.counts["points"] > 4 * _ffi.SORT_TILE and int(want["contours"][:, 1].max()) > 256 and got.counts["open_contours"] == 0
    assert got.stats["sort_passes"] == 4 + 2 and got.stats["rank_rounds"] >= 9      # 28 key bits for 10242 vertices, 9 for 300 layers


def test_two_runs_and_device_inputs(res, big):
    import torch
    v, t, h, want = big
    a, b = res.slice_mesh(v, t, O, S, 2, heights=h), res.slice_mesh(v, t, O, S, 2, heights=h)
    assert a.counts == b.counts and a.stats == b.stats
    for x, y in ((a.points, b.points), (a.contours, b.contours), (a.layer_first, b.layer_first)):
        assert np.array_equal(x, y)
    dev = torch.device("cuda", 0)
    dv, dt = torch.from_numpy(v).to(dev), torch.from_numpy(t.view(np.int32)).to(dev)
    d = res.slice_mesh(dv, dt, O, S, 2, heights=h, device=True)
    assert d.points.is_cuda and d.contours.is_cuda
    same(d, want, "device in, device out")
    same(res.slice_mesh(mesh.Mesh(dv, dt), None, O, S, 2, heights=h), want, "a Mesh of tensors")


def test_permutation_rotation_and_reversal(res):
    v, t, h = CASES["sphere"]
    rng = np.random.default_rng(11)
    rolled = np.stack([np.roll(row, int(k)) for row, k in zip(t[rng.permutation(len(t))], rng.integers(0, 3, len(t)))])
    for w in range(3):
        base = res.slice_mesh(v, t, O, S, w, heights=h)
        assert R.canonical_loops(as_result(res.slice_mesh(v, rolled, O, S, w, heights=h))) == R.canonical_loops(as_result(base))
        rev = res.slice_mesh(v, np.ascontiguousarray(t[:, ::-1]), O, S, w, heights=h)
        assert [rev.area(k) for k in range(len(h))] == [-base.area(k) for k in range(len(h))]


def test_out_of_range_indices_and_nan_corners(res):
    v, t, h = CASES["box"]
    v2 = np.concatenate([v, np.array([[np.nan, 1, 1], [1e9, 0, 0], [0, np.inf, 0]], dtype=np.float32)])
    t2 = np.concatenate([np.array([(0, 1, 99), (0, 1, 8)], dtype=np.uint32), t,
                         np.array([(2, 9, 3), (4, 4, 5), (10, 1, 2), (0xFFFFFFFF, 1, 2)], dtype=np.uint32)])
    for w in range(3):
        want = R.slice_mesh(v2, t2, O, S, w, h)
        assert want["counts"]["rejected"] == 6
        same(res.slice_mesh(v2, t2, O, S, w, heights=h), want, "rejected %d" % w)
    every = res.slice_mesh(v2, np.array([(0, 1, 99), (4, 4, 5)], dtype=np.uint32), O, S, 2, heights=h)     # nothing accepted
    assert every.counts["rejected"] == 2 and every.counts["points"] == 0 and every.numpy().layer_first.tolist() == [0] * 5


def test_one_layer_and_layers_that_miss(res):
    v, t, _ = CASES["torus"]
    for h in ([5.5], [-3.0], [-3.0, 1.0, 50.0], [2.0, 3.0, 40.0, 41.0, 42.0]):
        same(res.slice_mesh(v, t, O, S, 2, heights=h), R.slice_mesh(v, t, O, S, 2, h), "heights %s" % (h,))
    empty = res.slice_mesh(v, t, O, S, 2, heights=[-3.0, 60.0])
    assert empty.counts["points"] == 0 and empty.counts["contours"] == 0 and len(empty.points) == 0
    assert empty.numpy().layer_first.tolist() == [0, 0, 0] and empty.counts["paired_edges"] == 864


def test_layer_height_and_box(res):
    v, t, _ = CASES["sphere"]
    s = res.slice_mesh_box(v, t, axis="z", layer_height=0.75, resolution=512)
    lo, hi = v.min(axis=0), v.max(axis=0)
    assert len(s.heights) == int(np.ceil((hi[2] - lo[2]) / 0.75 - 0.5)) and s.counts["open_contours"] == 0 and s.counts["border_edges"] == 0
    step = float(np.max(hi.astype(np.float64) - lo)) / 511
    same(s, R.slice_mesh(v, t, lo, (step,) * 3, 2, s.heights), "box frame")
    with pytest.raises(ValueError):
        res.slice_mesh(v, None, O, S, 2, heights=[1.0])                       # a soup


def test_isolation(res):
    """A retained voxel, class mesh or topology result survives the call; the slices are those of the last slice call of either kind."""
    bv, bt, bh = CASES["box"]
    vox = res.voxelize_mesh(bv, bt, O, S, (16, 16, 16))
    occ = vox.occupancy().copy()
    cm = res.mesh_classes(occ, 1)
    cm_v = cm.vertices.copy()
    topo = res.label_occupancy(occ)
    labels = topo.labels().copy()
    a = res.slice_mesh(bv, bt, O, S, 2, heights=bh)
    assert np.array_equal(vox.occupancy(), occ) and np.array_equal(topo.labels(), labels)
    cm.read()
    assert np.array_equal(cm.vertices, cm_v)
    # rm_slice_contours replaces the mesh's slices and the other way round: rm_read_slices gives the last call's
    cc, words = csg.serialize(csg.scene("g1"))
    res.set_program(cc, words)
    pts = np.empty((a.counts["points"], 3), np.float32)
    c = res.slice_contours((-2.0,) * 3, (2.0,) * 3, 33, heights=[0.1, 0.4], axis=1)
    n = np.empty((len(c.points), 3), np.float32)
    res._read_into(res._L.rm_read_slices, (n.ctypes.data, 0, 0, 0, 0))
    assert np.array_equal(n, c.points)
    b = res.slice_mesh(bv, bt, O, S, 2, heights=bh)
    res._read_into(res._L.rm_read_slices, (pts.ctypes.data, 0, 0, 0, 0))
    assert np.array_equal(pts, a.points) and np.array_equal(b.points, a.points)
    with pytest.raises(_ffi.RmError) as e:                                      # normals and ids: the call computed none
        res._read_into(res._L.rm_read_slices, (0, 0, 0, n.ctypes.data, 0))
    assert e.value.status == _ffi.RM_ERR_ARG


def test_refusals_leave_the_previous_slices(res):
    v, t, h = CASES["box"]
    prev = res.slice_mesh(v, t, O, S, 0, heights=h)
    L, u64 = res._L, C.c_uint64
    counts, stats = (u64 * _ffi.RM_MSLICE_COUNTS)(), (u64 * _ffi.RM_MSLICE_STATS)()
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    good = dict(xyz=vp(v), nv=len(v), tri=vp(t), nt=len(t), dev=0, stream=None, o=fp(f(O)), s=fp(f(S)), axis=2, h=fp(f(h)), nl=len(h), flags=0,
                counts=counts, nc=_ffi.RM_MSLICE_COUNTS, stats=stats, ns=_ffi.RM_MSLICE_STATS)
    nan_h, far_h, down_h, same_h = f([3, np.nan, 7, 20]), f([3, 5, 7, 5000]), f([3, 7, 5, 20]), f([3, 5, 5.001, 20])
    bad_o, bad_s = f([0, np.inf, 0]), f([1, 0, 1])
    refusals = [(dict(xyz=None), _ffi.RM_ERR_NULL), (dict(tri=None), _ffi.RM_ERR_NULL), (dict(h=None), _ffi.RM_ERR_NULL),
                (dict(counts=None), _ffi.RM_ERR_NULL), (dict(nc=_ffi.RM_MSLICE_COUNTS - 1), _ffi.RM_ERR_ARG),
                (dict(ns=_ffi.RM_MSLICE_STATS - 1), _ffi.RM_ERR_ARG), (dict(flags=1), _ffi.RM_ERR_ARG), (dict(axis=3), _ffi.RM_ERR_ARG),
                (dict(o=fp(bad_o)), _ffi.RM_ERR_ARG), (dict(s=fp(bad_s)), _ffi.RM_ERR_ARG), (dict(nv=0), _ffi.RM_ERR_ARG),
                (dict(nl=0), _ffi.RM_ERR_RANGE), (dict(nl=65537), _ffi.RM_ERR_RANGE), (dict(nt=0), _ffi.RM_ERR_RANGE),
                (dict(nt=(1 << 28) + 1), _ffi.RM_ERR_RANGE), (dict(h=fp(nan_h)), _ffi.RM_ERR_ARG), (dict(h=fp(far_h)), _ffi.RM_ERR_RANGE),
                (dict(h=fp(down_h)), _ffi.RM_ERR_ARG), (dict(h=fp(same_h)), _ffi.RM_ERR_ARG),
                (dict(xyz=C.c_void_p(v.ctypes.data + 2), dev=1), _ffi.RM_ERR_ARG)]
    order = ("xyz", "nv", "tri", "nt", "dev", "stream", "o", "s", "axis", "h", "nl", "flags", "counts", "nc", "stats", "ns")
    pts = np.empty_like(prev.points)
    for change, status in refusals:
        a = dict(good, **change)
        assert L.rm_slice_mesh(res._h, *[a[k] for k in order]) == status, change
        pts[:] = 0
        res._read_into(L.rm_read_slices, (pts.ctypes.data, 0, 0, 0, 0))
        assert np.array_equal(pts, prev.points), change
    # each status outranks the ones after it
    both = dict(good, flags=1, nl=0, h=fp(nan_h))
    assert L.rm_slice_mesh(res._h, *[both[k] for k in order]) == _ffi.RM_ERR_ARG
    both = dict(good, nl=65537, h=fp(nan_h))
    assert L.rm_slice_mesh(res._h, *[both[k] for k in order]) == _ffi.RM_ERR_RANGE
    assert L.rm_slice_mesh(res._h, *[good[k] for k in order]) == _ffi.RM_OK


def test_command_line(res, tmp_path, capsys):
    import json
    v, t = VR.icosphere(2, 5.0, (1.0, 2.0, 3.0))
    stl, svg, cli = str(tmp_path / "part.stl"), str(tmp_path / "out.svg"), str(tmp_path / "out.cli")
    mesh.write(mesh.Mesh(v, t), stl)
    assert slicer.main(["--mesh", stl, "--axis", "z", "--layer-height", "0.5", "--fail-on", "open_contours>0,branch_edges>0,border_edges>0", svg]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["border_edges"] == 0 and out["open_contours"] == 0 and out["contours"] == out["layers"] == 20 and "<path" in open(svg).read()
    opened = str(tmp_path / "open.stl")
    mesh.write(mesh.Mesh(v, t[5:]), opened)
    assert slicer.main(["--mesh", opened, "--axis", "z", "--layer-height", "0.5", "--fail-on", "border_edges>0", cli]) == 2
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["border_edges"] > 0 and "$$LAYER" in open(cli).read()


def test_round_trip_against_slice_contours(res):
    """extract_mesh of g1 -> weld -> slice_mesh against slice_contours of g1 in the same planes: as many closed contours per layer,
    and layer areas within ROUND_TRIP_MARGIN."""
    cc, words = csg.serialize(csg.scene("g1"))
    res.set_program(cc, words)
    lo, hi, n = (-2.5,) * 3, (2.5,) * 3, 129
    m = mesh.weld(res.extract_mesh(lo, hi, n, normals=False, ids=False))
    heights = np.float32(-0.8) + np.arange(9, dtype=np.float32) * np.float32(0.2)
    step = 5.0 / (n - 1)
    for axis in (1, 2):
        c = res.slice_contours(lo, hi, n, heights=heights, axis=axis)
        s = res.slice_mesh(m, None, lo, (step,) * 3, axis, heights=heights)
        assert s.counts["border_edges"] == 0 and s.counts["branch_edges"] == 0 and s.counts["open_contours"] == 0
        for k in range(len(heights)):
            closed_c = sum(1 for _, closed in c.layer(k) if closed)
            assert len(s.layer(k)) == closed_c and len(c.layer(k)) == closed_c, (axis, k)
            a, b = s.area(k), c.area(k)
            print("axis %d layer %d: mesh %.6f lattice %.6f rel %.2e" % (axis, k, a, b, abs(a - b) / b))
            assert abs(a - b) <= ROUND_TRIP_MARGIN * b, (axis, k)
