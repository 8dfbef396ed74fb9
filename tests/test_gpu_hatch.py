"""Hatching on the GPU (rm_hatch_slices, rm_read_hatch).  The reference is always tests/hatch_ref.py applied to
the points and contours READ BACK with rm_read_slices (the slices' own correctness is other tests' business), and == means: the
counts, the segments as uint32, line and layer_first.  The known-answer meshes on all three axes in four directions, a level-5
icosphere in 300 layers (several sort tiles, seven sort passes, more than one block in both scans), segments that cross 20 000 lines,
line sets that miss everything, both producers of slices, open contours, zigzag, two runs, a device read, the slices and the other
retained results untouched, a new slicing call invalidating the hatch, and every refusal with the previous hatch still readable."""
import ctypes as C

import numpy as np
import pytest

import hatch_ref as H
import mesh_slice_ref as R
import voxel_ref as VR
from ray_marching_amd import _ffi, csg, renderer, slicer

pytestmark = pytest.mark.gpu

O, S = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
CASES = R.cases()
COS30 = (np.float32(np.cos(np.radians(30.0))), np.float32(np.sin(np.radians(30.0))))
DIRECTIONS = ((1.0, 0.0), (0.0, 1.0), COS30, (3.0, -4.0))
KNOWN = [("box", 2, (1, 0, 0.5, 1), 12, (24, 12, 0)), ("box", 2, (0, 1, -11.5, 1), 12, (32, 16, None)),
         ("torus", 2, (1, 0, -10.25, 0.5), 64, (112, 56, None)), ("open_box", 0, (1, 0, 0.5, 1), 12, (8, 4, 0)),
         ("open_box", 0, (0, 1, -11.5, 1), 12, (6, 0, 6)), ("open_box", 0, (1, 1, -20.25, 0.5), 80, (28, 8, 12)),
         ("fin", 0, (1, 0, 0.5, 1), 12, (10, 4, 2)), ("fin", 2, (1, 0, 0.5, 1), 12, (12, 6, 0)),
         ("sphere", 1, (np.float32(0.8660254), 0.5, -30, 0.37), 200, (2922, 1461, 0))]


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    yield r
    r.close()


def reference(s, lines, n_lines, zigzag=False):
    g = s.numpy()
    return H.hatch(g.points, g.contours, len(g.heights), g.axis, lines, n_lines, zigzag)


def same(got, want, what=""):
    g = got.numpy()
    print("%s: counts %s; stats %s" % (what, got.counts, got.stats))
    assert got.counts == want["counts"], what
    assert g.segments.dtype == np.float32 and g.segments.shape == want["segments"].shape, what
    assert np.array_equal(g.segments.view(np.uint32), want["segments"].view(np.uint32)), what
    assert np.array_equal(g.line, want["line"]) and np.array_equal(g.layer_first, want["layer_first"]), what
    assert got.stats["scratch_bytes"] > 0


def covering_lines(s, d, n_target):
    """About n_target lines across the points' s range, a little beyond both ends (one set for all layers)."""
    u, v = s.in_plane_axes
    p = s.numpy().points
    sv = H.normal_coordinate(p[:, u], p[:, v], np.float32(d[0]), np.float32(d[1])) if len(p) else np.array([0.0, 1.0])
    spacing = np.float32((sv.max() - sv.min()) / n_target)
    return H.as_lines((d[0], d[1], np.float32(sv.min() - 1.25 * float(spacing)), spacing), len(s.heights)), n_target + 4


@pytest.mark.parametrize("name", sorted(CASES))
def test_small_cases_on_three_axes_in_four_directions(res, name):
    v, t, h = CASES[name]
    for w in range(3):
        s = res.slice_mesh(v, t, O, S, w, heights=h)
        for d in DIRECTIONS:
            lines, n_lines = covering_lines(s, d, 24)
            want = reference(s, lines, n_lines)
            assert want["counts"]["crossings"] > 0
            same(res.hatch_slices(lines, n_lines), want, "%s %d %s" % (name, w, d))


def test_known_answers_ties_and_open_contours(res):
    for name, w, line, n_lines, (crossings, segments, odd) in KNOWN:
        v, t, h = CASES[name]
        s = res.slice_mesh(v, t, O, S, w, heights=h)
        lines = H.as_lines(line, len(h))
        got = res.hatch_slices(lines, n_lines)
        same(got, reference(s, lines, n_lines), "%s %d %s" % (name, w, line))
        assert (got.counts["crossings"], got.counts["segments"]) == (crossings, segments) and (odd is None or got.counts["odd_lines"] == odd)
    # a tie: a line through the point where fin's open contour ends on the box's outline (tests/test_hatch_cpu.py)
    v, t, h = CASES["fin"]
    s = res.slice_mesh(v, t, O, S, 2, heights=h)
    lines = H.as_lines((1, 1, 4.51171875 - 10.0, 1), 1)
    want = reference(s, lines, 8)
    assert want["ties"] >= 1
    same(res.hatch_slices(lines, 8), want, "tie")
    # r of both signs on one line: the direction (-3, 4) through a box about the origin
    bv, bt = VR.box((-6, -5, -4), (7, 9, 8))
    s = res.slice_mesh(bv, bt, O, S, 2, heights=[1.0, 2.0])
    lines, n_lines = covering_lines(s, (-3.0, 4.0), 40)
    want = reference(s, lines, n_lines)
    g = want["segments"].astype(np.float64)
    r0, r1 = g[:, 0] * -3.0 + g[:, 1] * 4.0, g[:, 2] * -3.0 + g[:, 3] * 4.0
    assert np.any((r0 < 0) & (r1 > 0))
    same(res.hatch_slices(lines, n_lines), want, "both signs")


@pytest.fixture(scope="module")
def big():
    v, t = VR.icosphere(5, 100.0, (120.3, 119.2, 121.1))
    return v, t, 21.7 + np.arange(300) * 0.66


def test_sort_and_scan_boundaries(res, big):
    v, t, h = big
    s = res.slice_mesh(v, t, O, S, 2, heights=h)
    lines, n = slicer.hatch_lines(s, 1.0, 45.0, 67.0)
    assert n <= 300
    got = res.hatch_slices(lines, 300)
    same(got, reference(s, lines, 300), "icosphere 5")
    c = got.counts
    assert c["crossings"] > 4 * _ffi.SORT_TILE and len(h) * 300 > 1 << 16 and got.stats["sort_passes"] == -(-(32 + 17) // 8) == 7
    assert len(s.points) > 1024 and c["crossings"] > 1024 and c["odd_lines"] == 0       # both scans run over more than one block


def test_long_segments_and_lines_that_miss(res):
    """A box 200 x 3 cut 1 / 128 above its floor: the long faces' outline splits at their diagonals 0.4 from a corner, so two
    segments cross about 19 960 of the 2^15 lines each -- far more items than a sort tile or a scan block holds.  Then lines whose
    c lies beyond the box altogether."""
    v, t = VR.box((0, 0, 0), (200, 3, 4))
    s = res.slice_mesh(v, t, O, S, 2, heights=[0.004])
    lines = H.as_lines((0, 1, -210.0, 0.01), 1)
    want = reference(s, lines, 1 << 15)
    got = res.hatch_slices(lines, 1 << 15)
    same(got, want, "long")
    tail, head, _ = H.tails_and_heads(s.contours, len(s.points))
    per_segment = np.abs(s.points[tail, 0].astype(np.float64) - s.points[head, 0]) / 0.01
    assert np.sort(per_segment)[-2] > 19000 and 39000 < got.counts["crossings"] < 41000 and got.counts["odd_lines"] == 0
    before = got.numpy()
    miss = H.as_lines((0, 1, 1000.0, 0.01), 1)
    empty = res.hatch_slices(miss, 1 << 15)
    same(empty, reference(s, miss, 1 << 15), "miss")
    e = empty.numpy()
    assert empty.counts["crossings"] == 0 and e.segments.shape == (0, 4) and e.line.shape == (0,) and e.layer_first.tolist() == [0, 0]
    assert empty.counts["segments_in"] == len(s.points) and before.counts["segments"] > 0


def test_both_producers(res):
    cc, words = csg.serialize(csg.scene("g8"))
    res.set_program(cc, words)
    s = res.slice_contours((-3.0,) * 3, (3.0,) * 3, 96, heights=[-50.0, -0.3, 60.0, 0.2, 70.0], axis=1)
    assert np.diff(s.layer_first.astype(np.int64)).tolist()[0::2] == [0, 0, 0] and len(s.points) > 0
    for angle in (0.0, 33.0):
        lines, n_lines = slicer.hatch_lines(s, 0.02, angle, 90.0)
        got = res.hatch_slices(lines, n_lines)
        same(got, reference(s, lines, n_lines), "slice_contours %g" % angle)
        lf = got.layer_first.astype(np.int64)
        assert lf[1] == 0 and lf[2] == lf[3] and lf[4] == lf[5] and lf[2] > 0 and got.counts["segments"] > 100
    v, t, h = CASES["torus"]
    m = res.slice_mesh(v, t, O, S, 2, heights=[-9.0, 5.0, 5.5, 6.0, 44.0])
    lines, n_lines = slicer.hatch_lines(m, 0.3, 45.0, 90.0)
    same(res.hatch_slices(lines, n_lines), reference(m, lines, n_lines), "slice_mesh")


def test_zigzag(res):
    v, t, h = CASES["sphere"]
    s = res.slice_mesh(v, t, O, S, 1, heights=h)
    lines = H.as_lines((np.float32(0.8660254), 0.5, -30, 0.37), len(h))
    plain, zig = res.hatch_slices(lines, 200), res.hatch_slices(lines, 200, zigzag=True)
    same(zig, reference(s, lines, 200, True), "zigzag")
    same(plain, reference(s, lines, 200), "plain")
    assert not np.array_equal(plain.segments, zig.segments) and np.array_equal(plain.line, zig.line)


def test_determinism_and_plumbing(res, big):
    import torch
    v, t, h = big
    s = res.slice_mesh(v, t, O, S, 2, heights=h)
    lines, _ = slicer.hatch_lines(s, 1.0, 45.0, 67.0)
    a, b = res.hatch_slices(lines, 300), res.hatch_slices(lines, 300)
    assert a.counts == b.counts and a.stats == b.stats
    for x, y in ((a.segments, b.segments), (a.line, b.line), (a.layer_first, b.layer_first)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    d = res.hatch_slices(lines, 300, device=True)
    assert d.segments.is_cuda and d.line.is_cuda and d.layer_first.is_cuda
    torch.cuda.synchronize()
    g = d.numpy()
    assert np.array_equal(g.segments.view(np.uint32), a.segments.view(np.uint32)) and np.array_equal(g.line, a.line)
    assert np.array_equal(g.layer_first, a.layer_first)
    # the slices after the hatch: byte for byte what they were
    pts, con, lf = np.empty_like(s.points), np.empty_like(s.contours), np.empty_like(s.layer_first)
    res._read_into(res._L.rm_read_slices, (pts.ctypes.data, con.ctypes.data, lf.ctypes.data, 0, 0))
    assert pts.tobytes() == s.points.tobytes() and con.tobytes() == s.contours.tobytes() and lf.tobytes() == s.layer_first.tobytes()


def test_isolation_and_invalidation(res):
    """Voxels, labels and a class mesh survive the hatch; a new slicing call of either kind makes the hatch unreadable."""
    bv, bt, bh = CASES["box"]
    vox = res.voxelize_mesh(bv, bt, O, S, (16, 16, 16))
    occ = vox.occupancy().copy()
    cm = res.mesh_classes(occ, 1)
    cm_v = cm.vertices.copy()
    topo = res.label_occupancy(occ)
    labels = topo.labels().copy()
    s = res.slice_mesh(bv, bt, O, S, 2, heights=bh)
    lines = H.as_lines((1, 0, 0.5, 1), len(bh))
    got = res.hatch_slices(lines, 12)
    assert np.array_equal(vox.occupancy(), occ) and np.array_equal(topo.labels(), labels)
    cm.read()
    assert np.array_equal(cm.vertices, cm_v)
    seg = np.zeros_like(got.segments)
    res._read_into(res._L.rm_read_hatch, (seg.ctypes.data, 0, 0))
    assert np.array_equal(seg, got.segments)
    cc, words = csg.serialize(csg.scene("g1"))
    res.set_program(cc, words)
    for again in (lambda: res.slice_mesh(bv, bt, O, S, 2, heights=bh), lambda: res.slice_contours((-2.0,) * 3, (2.0,) * 3, 33, heights=[0.1], axis=1)):
        again()
        with pytest.raises(_ffi.RmError) as e:
            res._read_into(res._L.rm_read_hatch, (seg.ctypes.data, 0, 0))
        assert e.value.status == _ffi.RM_ERR_ARG
        s2 = res.slice_mesh(bv, bt, O, S, 2, heights=bh)
        same(res.hatch_slices(lines, 12), reference(s2, lines, 12), "after a new slicing")
    fresh = renderer.RayMarchingResources(0)
    try:
        with pytest.raises(_ffi.RmError) as e:
            fresh.hatch_slices(lines, 12)                                           # nothing has been sliced
        assert e.value.status == _ffi.RM_ERR_ARG
        with pytest.raises(_ffi.RmError) as e:
            fresh._read_into(fresh._L.rm_read_hatch, (seg.ctypes.data, 0, 0))
        assert e.value.status == _ffi.RM_ERR_ARG
    finally:
        fresh.close()


def test_refusals_in_order_leave_the_previous_hatch(res):
    v, t, _ = CASES["sphere"]
    h = 3.0 + np.arange(300) * 0.06                                                 # 300 layers: 300 x 2^24 lines exceed 2^32
    s = res.slice_mesh(v, t, O, S, 2, heights=h)
    lines, n_lines = slicer.hatch_lines(s, 0.5)
    prev = res.hatch_slices(lines, n_lines)
    L, u64 = res._L, C.c_uint64
    counts, stats = (u64 * _ffi.RM_HATCH_COUNTS)(), (u64 * _ffi.RM_HATCH_STATS)()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731

    def changed(row, column, value):
        a = lines.copy()
        a[row, column] = value
        return a
    bad = {"nan": changed(7, 2, np.nan), "inf": changed(299, 0, np.inf), "zero": changed(0, 3, 0.0), "negative": changed(150, 3, -0.5),
           "direction": np.concatenate([lines[:10], [[0.0, 0.0, 1.0, 1.0]], lines[11:]]).astype(np.float32)}
    good = dict(lines=fp(lines), nl=len(lines), n=n_lines, flags=0, counts=counts, nc=_ffi.RM_HATCH_COUNTS, stats=stats, ns=_ffi.RM_HATCH_STATS)
    refusals = [(dict(lines=None), _ffi.RM_ERR_NULL), (dict(counts=None), _ffi.RM_ERR_NULL), (dict(stats=None), _ffi.RM_ERR_NULL),
                (dict(nc=_ffi.RM_HATCH_COUNTS - 1), _ffi.RM_ERR_ARG), (dict(ns=_ffi.RM_HATCH_STATS - 1), _ffi.RM_ERR_ARG),
                (dict(flags=2), _ffi.RM_ERR_ARG), (dict(flags=0x80000001), _ffi.RM_ERR_ARG), (dict(nl=299), _ffi.RM_ERR_ARG),
                (dict(nl=0), _ffi.RM_ERR_ARG)]
    refusals += [(dict(lines=fp(a)), _ffi.RM_ERR_ARG) for a in bad.values()]
    refusals += [(dict(n=0), _ffi.RM_ERR_RANGE), (dict(n=(1 << 24) + 1), _ffi.RM_ERR_RANGE), (dict(n=1 << 24), _ffi.RM_ERR_RANGE)]
    order = ("lines", "nl", "n", "flags", "counts", "nc", "stats", "ns")
    seg, pts = np.empty_like(prev.segments), np.empty_like(s.points)
    for change, status in refusals:
        a = dict(good, **change)
        assert L.rm_hatch_slices(res._h, *[a[k] for k in order]) == status, change
        seg[:], pts[:] = 0, 0
        res._read_into(L.rm_read_hatch, (seg.ctypes.data, 0, 0))
        res._read_into(L.rm_read_slices, (pts.ctypes.data, 0, 0, 0, 0))
        assert np.array_equal(seg.view(np.uint32), prev.segments.view(np.uint32)) and np.array_equal(pts, s.points), change
    # each status outranks the ones after it
    for both, status in ((dict(lines=None, nc=0, n=0), _ffi.RM_ERR_NULL), (dict(flags=2, n=0), _ffi.RM_ERR_ARG),
                         (dict(lines=fp(bad["nan"]), n=(1 << 24) + 1), _ffi.RM_ERR_ARG), (dict(nl=299, n=0), _ffi.RM_ERR_ARG)):
        a = dict(good, **both)
        assert L.rm_hatch_slices(res._h, *[a[k] for k in order]) == status, both
    assert L.rm_hatch_slices(res._h, *[good[k] for k in order]) == _ffi.RM_OK
    with pytest.raises(_ffi.RmError) as e:                                          # a misaligned device destination
        res._read_into(L.rm_read_hatch, (4, 0, 0), device=True)
    assert e.value.status == _ffi.RM_ERR_ARG


def test_command_line(res, tmp_path, capsys):
    import json
    from ray_marching_amd import mesh
    v, t = VR.icosphere(2, 5.0, (1.0, 2.0, 3.0))
    stl, svg, cli = str(tmp_path / "part.stl"), str(tmp_path / "out.svg"), str(tmp_path / "out.cli")
    mesh.write(mesh.Mesh(v, t), stl)
    assert slicer.main(["--mesh", stl, "--axis", "z", "--layer-height", "0.5", "--hatch", "0.4", "--zigzag", "--fail-on", "odd_lines>0", cli]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["odd_lines"] == 0 and out["hatch_segments"] > 100 and out["crossings"] == 2 * out["hatch_segments"] and out["segments"] > 0
    assert open(cli).read().count("$$HATCHES/1,") == out["layers"] == 20
    assert slicer.main(["--scene", "g1", "--res", "64", "--layer-height", "0.5", "--lo", "-2", "--hi", "2", "--hatch", "0.1", "--hatch-angle", "30",
                        "--hatch-rotate", "60", "--fail-on", "lines_hit>0", svg]) == 2
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["lines_hit"] > 0 and '<path fill="none"' in open(svg).read()
