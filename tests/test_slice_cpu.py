"""Slicing without a GPU: the library's case table against the numpy restatement (tests/slice_ref.py), the restatement's
chains on numpy-oracle fields, the SVG / CLI writers, the Python argument checks, and the C, Rust and Python faces of the
new ABI (tests/test_gpu_slice.py runs the kernels)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scenes
import slice_ref as R
from oracle import rm_oracle_np as onp
from ray_marching_amd import _ffi, renderer
from ray_marching_amd import slicer as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SLICE_FUNCTIONS = ("rm_slice_contours", "rm_read_slices", "rm_slice_case_table")


def lib_table():
    out = np.zeros(80, dtype=np.uint32)
    assert _ffi.hip_lib().rm_slice_case_table(out.ctypes.data, 80) == _ffi.RM_OK
    return out.reshape(16, 5)


# ---- the case table --------------------------------------------------------------------------------------------------------
def test_case_table_matches_the_restated_rule():
    lib, ref = lib_table(), R.table()
    for case in range(16):
        assert np.array_equal(lib[case], ref[case]), (case, lib[case], ref[case])
    assert lib[0, 0] == 0 and lib[15, 0] == 0
    assert sorted(np.nonzero(lib[:, 0] == 2)[0].tolist()) == [6, 9]
    # the complement of a case is the same segments, reversed
    for case in range(1, 15):
        a = {(int(t), int(h)) for t, h in lib[case, 1:1 + 2 * lib[case, 0]].reshape(-1, 2)}
        b = {(int(h), int(t)) for t, h in lib[15 - case, 1:1 + 2 * lib[15 - case, 0]].reshape(-1, 2)}
        if case not in (6, 9):
            assert a == b, case
        else:       # the diagonal cases cut off their inside corners: the complement joins the other pair of edges
            assert {frozenset(x) for x in a}.isdisjoint({frozenset(x) for x in b}), case


def test_case_table_anchors():
    lib = lib_table()
    nil = R.NO_EDGE
    assert list(lib[1]) == [1, 0, 2, nil, nil]
    assert list(lib[6]) == [2, 2, 1, 3, 0]
    assert list(lib[9]) == [2, 0, 2, 1, 3]


def test_case_table_arguments_and_null_contexts():
    L = _ffi.hip_lib()
    small = np.zeros(79, dtype=np.uint32)
    assert L.rm_slice_case_table(small.ctypes.data, 79) == _ffi.RM_ERR_ARG
    assert L.rm_slice_case_table(None, 80) == _ffi.RM_ERR_NULL
    o, s, h = (C.c_float * 2)(0, 0), (C.c_float * 2)(1, 1), (C.c_float * 1)(0)
    counts = (C.c_uint64 * 2)()
    out = np.zeros(64, dtype=np.float32)
    assert L.rm_slice_contours(None, 1, o, s, 4, 4, h, 1, 0.0, 0, counts, 2) == _ffi.RM_ERR_NULL
    assert L.rm_read_slices(None, out.ctypes.data, None, None, None, None, 0, None) == _ffi.RM_ERR_NULL


def test_the_inside_lies_on_the_left_of_every_segment():
    # mid-points of the cell's edges in (u, v): bottom, top, left, right
    mid = np.array([[0.5, 0.0], [0.5, 1.0], [0.0, 0.5], [1.0, 0.5]])
    lib = lib_table()
    for case in range(1, 15):
        for t, h in lib[case, 1:1 + 2 * lib[case, 0]].reshape(-1, 2):
            a, d = mid[t], mid[h] - mid[t]
            left = [c for c in range(4) if d[0] * ((c >> 1) - a[1]) - d[1] * ((c & 1) - a[0]) > 0]
            # every corner strictly on the left of a segment that is alone in its cell is inside; of the two segments of a
            # diagonal case each has exactly its own inside corner on the left
            if lib[case, 0] == 1:
                assert left and all((case >> c) & 1 for c in left), (case, t, h)
                assert not any((case >> c) & 1 for c in range(4) if c not in left), (case, t, h)
            else:
                assert len(left) == 1 and (case >> left[0]) & 1, (case, t, h)


# ---- the restatement on numpy-oracle fields --------------------------------------------------------------------------------------
def oracle_layers(cc, w, axis, origin_uv, step_uv, shape_uv, heights, max_dist=100.0):
    out = []
    for h in heights:
        p = R.layer_points(axis, origin_uv, step_uv, shape_uv, h)
        with np.errstate(all="ignore"):
            d = onp.map_scene(cc, w, F(max_dist), p[:, 0], p[:, 1], p[:, 2])
        out.append(np.asarray(d, dtype=F).reshape(shape_uv[1], shape_uv[0]))
    return out


def check_partition(points, contours, layer_first, n_layers):
    """Every point is in exactly one contour, contours are back to back, layers in order."""
    assert len(layer_first) == n_layers + 1 and layer_first[0] == 0 and layer_first[-1] == len(contours)
    assert np.all(np.diff(layer_first.astype(np.int64)) >= 0)
    first, count = contours[:, 0].astype(np.int64), contours[:, 1].astype(np.int64)
    assert np.array_equal(first, np.cumsum(count) - count) and int(count.sum()) == len(points)
    assert np.all(count[contours[:, 3] == 1] >= 4) and np.all(count >= 2)
    for k in range(n_layers):
        assert np.all(contours[layer_first[k]:layer_first[k + 1], 2] == k)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_circle_of_g1(oracle, axis):
    cc, w = oracle.serialize(*scenes.SCENES["g1"]())
    s = F(3.0) / F(64)
    origin, step, shape = (-1.5, -1.5), (s, s), (65, 65)
    pts, con, lf = R.slice_contours(oracle_layers(cc, w, axis, origin, step, shape, [0.3]), axis, origin, step, [0.3])
    check_partition(pts, con, lf, 1)
    assert len(con) == 1 and con[0, 3] == 1 and con[0, 1] == len(pts)
    assert np.all(pts[:, axis] == F(0.3))
    u, v = R.in_plane_axes(axis)
    uv = pts[:, [u, v]].astype(np.float64)
    area, rho, sd = R.shoelace(uv), np.sqrt(0.91), float(s)
    print("g1 through 0.3 on axis %d: %d points, area %.5f" % (axis, len(pts), area))
    assert np.pi * (rho - 2 * sd) ** 2 <= area <= np.pi * (rho + sd) ** 2
    assert np.all(np.abs(np.hypot(uv[:, 0], uv[:, 1]) - rho) <= sd)


@pytest.mark.parametrize("name, axis", [("g8", 0), ("g32", 1), ("xform_mix", 2), ("g32s", 1)])
def test_chains_partition_the_vertices(oracle, name, axis):
    all_scenes = dict(list(scenes.SCENES.items()) + list(scenes.EXT_SCENES.items()))
    cc, w = oracle.serialize(*all_scenes[name]())
    origin, step, shape = (-2.0, -1.5), (F(0.09), F(0.11)), (41, 37)
    heights = [0.1, -0.4, 0.1, 0.75]
    layers = oracle_layers(cc, w, axis, origin, step, shape, heights)
    n_vertices = 0
    for d in layers:
        uv, nxt, prv = R.layer_links(d, origin, step)
        n_vertices += len(uv)
        # as many chain starts as ends, and next / prev are inverse to each other
        assert np.count_nonzero(nxt == R.NIL) == np.count_nonzero(prv == R.NIL)
        has = nxt != R.NIL
        assert np.array_equal(prv[nxt[has]], np.nonzero(has)[0])
        ids = [v for chain, _ in R.layer_chains(nxt, prv) for v in chain]
        assert sorted(ids) == list(range(len(uv)))          # every vertex in exactly one contour
    pts, con, lf = R.slice_contours(layers, axis, origin, step, heights)
    assert len(pts) == n_vertices > 0
    check_partition(pts, con, lf, len(heights))
    # a duplicated height gives the same layer twice
    a = slice(int(lf[0]), int(lf[1]))
    b = slice(int(lf[2]), int(lf[3]))
    assert np.array_equal(con[a][:, 1], con[b][:, 1]) and np.array_equal(con[a][:, 3], con[b][:, 3])
    # open contours start and end on the lattice's border
    cu, cv = R.axis_coords(origin[0], step[0], shape[0]), R.axis_coords(origin[1], step[1], shape[1])
    u, v = R.in_plane_axes(axis)
    for first, count, _, closed in con.tolist():
        if not closed:
            for p in (pts[first], pts[first + count - 1]):
                assert p[u] in (cu[0], cu[-1]) or p[v] in (cv[0], cv[-1])


def test_outer_boundaries_run_counter_clockwise_and_holes_clockwise():
    n = 41
    s = F(3.0) / F(n - 1)
    cu = R.axis_coords(-1.5, s, n).astype(np.float64)
    r = np.hypot(cu[None, :], cu[:, None])
    d = np.maximum(r - 1.0, 0.5 - r).astype(F)          # an annulus: inside between the radii 0.5 and 1
    pts, con, lf = R.slice_contours([d], 2, (-1.5, -1.5), (s, s), [0.0])
    assert len(con) == 2 and np.all(con[:, 3] == 1)
    areas = [R.shoelace(pts[f:f + c, :2]) for f, c, _, _ in con.tolist()]
    assert max(areas) > 0 > min(areas)
    assert abs(max(areas) / np.pi - 1.0) < 0.02 and abs(-min(areas) / (0.25 * np.pi) - 1.0) < 0.05
    sl = S.Slices(pts, con, lf, [0.0], 2)
    assert abs(sl.area(0) / (0.75 * np.pi) - 1.0) < 0.02       # holes subtract


# ---- files ---------------------------------------------------------------------------------------------------------------
def small_slices(oracle):
    cc, w = oracle.serialize(*scenes.SCENES["g32"]())
    s = F(3.0) / F(63)
    origin, step, shape, heights = (-1.0, -1.0), (s, s), (64, 64), [0.1, 0.35]
    pts, con, lf = R.slice_contours(oracle_layers(cc, w, 1, origin, step, shape, heights), 1, origin, step, heights)
    assert np.any(con[:, 3] == 0) and np.any(con[:, 3] == 1)
    return S.Slices(pts, con, lf, heights, 1, lattice=(np.asarray(origin, F), np.asarray(step, F), shape))


def test_slices_accessors(oracle):
    sl = small_slices(oracle)
    assert sl.in_plane_axes == (2, 0)
    total = 0
    for k in range(2):
        layer = sl.layer(k)
        assert len(layer) == int(sl.layer_first[k + 1]) - int(sl.layer_first[k])
        total += len(layer)
    assert total == len(sl.contours)
    uv, closed = sl.contour(0)
    f, c = int(sl.contours[0, 0]), int(sl.contours[0, 1])
    assert np.array_equal(uv, sl.points[f:f + c][:, [2, 0]]) and closed == bool(sl.contours[0, 3])
    assert sl.numpy().points is sl.points
    assert sl.area(0) == sum(R.shoelace(uv) for uv, closed in sl.layer(0) if closed)


def parse_svg(path):
    text = open(path).read()
    layers = []
    for g in re.finditer(r'<g id="layer-(\d+)" data-height="([^"]+)">(.*?)</g>', text, re.S):
        contours = []
        paths = re.findall(r"<path ([^>]*)/>", g.group(3))
        assert len(paths) <= 1
        for attrs in paths:
            assert 'fill-rule="evenodd"' in attrs
            d = re.search(r'd="([^"]*)"', attrs).group(1)
            for sub in re.findall(r"M[^M]*", d):
                tokens = sub.split()
                closed = tokens[-1] == "Z"
                body = tokens[:-1] if closed else tokens
                assert body[0] == "M" and all(t == "L" for t in body[3::3])
                nums = [t for t in body if t not in ("M", "L")]
                contours.append((np.asarray(nums, dtype=np.float64).astype(F).reshape(-1, 2), closed))
        layers.append((int(g.group(1)), F(g.group(2)), contours))
    box = [float(x) for x in re.search(r'viewBox="([^"]*)"', text).group(1).split()]
    return layers, box


def test_svg_round_trip(oracle, tmp_path):
    sl = small_slices(oracle)
    p = str(tmp_path / "s.svg")
    S.write_svg(sl, p)
    layers, box = parse_svg(p)
    assert [k for k, _, _ in layers] == [0, 1]
    for k, h, contours in layers:
        assert h == sl.heights[k]
        want = sl.layer(k)
        assert len(contours) == len(want)
        for (uv, closed), (ruv, rclosed) in zip(contours, want):
            assert closed == rclosed and uv.tobytes() == ruv.tobytes()         # %.9g round-trips binary32
    (ou, ov), (su, sv), (nu, nv) = sl.lattice
    assert box[0] == float(ou) and box[2] == pytest.approx((nu - 1) * float(su)) and box[3] == pytest.approx((nv - 1) * float(sv))
    assert box[1] == pytest.approx(-(float(ov) + (nv - 1) * float(sv)))


def parse_cli(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "$$HEADERSTART" and "$$HEADEREND" in lines and lines[-2] == "$$GEOMETRYEND"
    n_layers = int(next(x for x in lines if x.startswith("$$LAYERS/")).split("/")[1])
    layers = []
    for line in lines[lines.index("$$GEOMETRYSTART") + 1:]:
        if line.startswith("$$LAYER/"):
            layers.append((F(line.split("/")[1]), []))
        elif line.startswith("$$POLYLINE/"):
            f = line.split("/")[1].split(",")
            ident, direction, n = int(f[0]), int(f[1]), int(f[2])
            xy = np.asarray(f[3:], dtype=np.float64).astype(F).reshape(-1, 2)
            assert ident == 1 and len(xy) == n
            layers[-1][1].append((direction, xy))
    assert len(layers) == n_layers
    return layers


def test_cli_round_trip(oracle, tmp_path):
    sl = small_slices(oracle)
    p = str(tmp_path / "s.cli")
    S.write_cli(sl, p)
    layers = parse_cli(p)
    assert len(layers) == 2
    seen = set()
    for k, (h, polys) in enumerate(layers):
        assert h == sl.heights[k]
        want = sl.layer(k)
        assert len(polys) == len(want)
        for (direction, xy), (ruv, rclosed) in zip(polys, want):
            seen.add(direction)
            if rclosed:
                assert direction in (0, 1)
                assert xy[:-1].tobytes() == ruv.tobytes() and xy[-1].tobytes() == ruv[0].tobytes()    # repeats its first point
                assert direction == (1 if R.shoelace(ruv) > 0 else 0)
            else:
                assert direction == 2 and xy.tobytes() == ruv.tobytes()
    assert 2 in seen and 1 in seen


def test_write_picks_the_format_by_extension(oracle, tmp_path):
    sl = small_slices(oracle)
    with pytest.raises(ValueError):
        S.write(sl, str(tmp_path / "s.stl"))
    S.write(sl, str(tmp_path / "s.SVG"))
    S.write(sl, str(tmp_path / "s.cli"))
    assert open(str(tmp_path / "s.SVG")).read().count("<path ") == 2


# ---- Python argument checks (raised before any device call) ----------------------------------------------------------------
class _NoDevice(renderer.RayMarchingResources):
    def __init__(self):       # the argument checks only: no context
        self._L, self._h, self.device = _ffi.hip_lib(), None, 0


@pytest.mark.parametrize("kw", [
    dict(lo=(-1, -1, -1), hi=(1, 1, 1), resolution=1, heights=[0.0]),
    dict(lo=(-1, -1, -1), hi=(1, 1, 1), resolution=(8, 1), heights=[0.0]),
    dict(lo=(-1, -1, -1), hi=(1, 1, 1), resolution=(8, 8, 8), heights=[0.0]),
    dict(lo=(-1, -1, -1), hi=(1, 1, 1), resolution=2.5, heights=[0.0]),
    dict(lo=(1, -1, -1), hi=(1, 1, 1), resolution=8, heights=[0.0]),
    dict(lo=(-1, -1, -1), hi=(1, 1, np.inf), resolution=8, heights=[0.0]),
    dict(lo=(-1, -1), hi=(1, 1), resolution=8, heights=[0.0]),
    dict(lo=-1, hi=1, resolution=8),                                          # neither heights nor layer_height
    dict(lo=-1, hi=1, resolution=8, heights=[0.0], layer_height=0.1),         # both
    dict(lo=-1, hi=1, resolution=8, heights=[]),
    dict(lo=-1, hi=1, resolution=8, heights=[0.0, np.nan]),
    dict(lo=-1, hi=1, resolution=8, layer_height=0.0),
    dict(lo=-1, hi=1, resolution=8, layer_height=-0.1),
    dict(lo=-1, hi=1, resolution=8, layer_height=np.inf),
    dict(lo=-1, hi=1, resolution=8, layer_height=1e-6),                       # more than 65536 layers
    dict(lo=-1, hi=1, resolution=8, heights=[0.0], axis=3),
    dict(lo=-1, hi=1, resolution=8, heights=[0.0], axis="w"),
    dict(lo=-1, hi=1, resolution=8, heights=[0.0], axis=1.0),
    dict(lo=-1, hi=1, resolution=8, heights=[0.0], level=np.nan),
])
def test_slice_contours_rejects_bad_arguments(kw):
    with pytest.raises(ValueError):
        _NoDevice().slice_contours(**kw)


@pytest.mark.parametrize("origin, step, shape, heights", [
    ((0, 0, 0), (1, 1), (4, 4), [0.0]), ((0, 0), (1, 0), (4, 4), [0.0]), ((0, 0), (1, -1), (4, 4), [0.0]),
    ((0, np.nan), (1, 1), (4, 4), [0.0]), ((0, 0), (1, 1), (4,), [0.0]), ((0, 0), (1, 1), (4, 1), [0.0]),
    ((0, 0), (1, 1), (4, 4), []), ((0, 0), (1, 1), (4, 4), [np.inf])])
def test_slice_contours_grid_rejects_bad_lattices(origin, step, shape, heights):
    with pytest.raises(ValueError):
        _NoDevice().slice_contours_grid(1, origin, step, shape, heights)


class _Recorder:
    """Stands in for the library: records what reaches rm_slice_contours, then fails the call."""

    def __init__(self):
        self.calls = []

    def rm_slice_contours(self, h, axis, o, s, nu, nv, heights, n_layers, level, flags, counts, n_counts):
        self.calls.append((axis, [o[0], o[1]], [s[0], s[1]], (nu, nv), [heights[k] for k in range(n_layers)], level, flags, n_counts))
        return _ffi.RM_ERR_ARG


def test_box_and_layer_height_reach_the_library_as_a_lattice():
    r = _NoDevice()
    rec = r._L = _Recorder()
    with pytest.raises(_ffi.RmError):
        r.slice_contours((-1.0, -2.0, -3.0), (2.0, 0.5, 1.0), (9, 17), layer_height=0.75, axis="y", level=0.25, normals=True)
    axis, o, s, n, heights, level, flags, n_counts = rec.calls[-1]
    # y up: u = z, v = x
    assert axis == 1 and o == [-3.0, -1.0] and s == [float(F(4.0) / F(8.0)), float(F(3.0) / F(16.0))] and n == (9, 17)
    want = [float(F(-2.0) + (F(k) + F(0.5)) * F(0.75)) for k in range(4)]           # mid-layer, while below hi
    assert heights == [h for h in want if h < 0.5] and len(heights) == 3
    assert level == 0.25 and flags == _ffi.RM_MESH_NORMALS and n_counts == _ffi.RM_SLICE_COUNTS
    with pytest.raises(_ffi.RmError):
        r.slice_contours(-2.5, 2.5, 64, heights=[0.5, -1.0, 0.5], axis=2, ids=True)
    axis, o, s, n, heights, level, flags, _ = rec.calls[-1]
    assert axis == 2 and o == [-2.5, -2.5] and s == [float(F(5.0) / F(63.0))] * 2 and n == (64, 64)
    assert heights == [0.5, -1.0, 0.5] and level == 0.0 and flags == _ffi.RM_MESH_IDS
    # strided views handed in directly
    strided = np.arange(4, dtype=F)[::2] + F(0.25)
    with pytest.raises(_ffi.RmError):
        r.slice_contours_grid(0, strided, np.broadcast_to(F(1.5), (2,)), (8, 9), np.arange(6, dtype=F)[::3])
    assert rec.calls[-1][:5] == (0, [0.25, 2.25], [1.5, 1.5], (8, 9), [0.0, 3.0])


# ---- the C, Rust and Python faces ------------------------------------------------------------------------------------------
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rm_abi.h")).read(), flags=re.S)


def rust_text():
    return open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()


def test_slice_symbols_and_constants():
    text, rust, L = header_text(), rust_text(), _ffi.hip_lib()
    for name in SLICE_FUNCTIONS:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
        assert re.search(r"pub fn %s\(" % name, rust), name
    body = re.search(r"enum\s+rm_slicecount\s*\{(.*?)\}", text, re.S).group(1)
    consts = {n: int(v) for n, v in re.findall(r"(RM_[A-Z0-9_]+)\s*=\s*(-?\d+)", body)}
    assert consts == {"RM_SLICE_POINTS": 0, "RM_SLICE_CONTOURS": 1, "RM_SLICE_COUNTS": 2}
    for name, value in consts.items():
        assert getattr(_ffi, name) == value
        assert re.search(r"pub const %s: c_int = %d;" % (name, value), rust), name
    assert re.search(r"#define RM_ABI_VERSION 2\b", text)
    assert L.rm_abi_version() == 2
    assert re.search(r"pub const RM_ABI_VERSION: c_int = 2;", rust)


def test_rust_wrappers_check_their_slices():
    rust = rust_text()
    assert re.search(r"pub fn slice_contours\(&self.*?\) -> Result<\(u64, u64\), RmError>", rust, re.S)
    # read_slices checks its slices against the counts of the context's own result, not against counts the caller passes
    assert re.search(r"pub fn read_slices\(&self, out_points: Option<&mut \[f32\]>", rust)
    body = rust[rust.index("pub fn read_slices("):]
    body = body[:body.index("\n    }\n")]
    assert "self.slices.get()" in body
    call = body.index("rm_read_slices(")
    for arg in ("out_points", "out_contours", "out_layer_first", "out_normals", "out_ids"):
        assert re.search(r"assert!\(%s\.as_ref\(\)" % arg, body[:call]), arg
    ext = rust[rust.index("pub fn slice_contours("):]
    ext = ext[:ext.index("\n    }\n")]
    assert ext.index("self.slices.set(None)") < ext.index("rm_slice_contours(") < ext.index("self.slices.set(Some(")
    assert "heights.len() as u32" in ext and "RM_SLICE_COUNTS as u32" in ext
