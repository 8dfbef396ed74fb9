"""Hatching without a GPU: the two restatements of hatch_ref against each other and against the known answers,
the properties the contract promises (even crossings, ends on their lines, midpoints inside, zigzag as a permutation),
slicer.hatch_lines, the files with and without a hatch, the command line's refusals, the three faces' constants, and
tests/cpp/hatch_layout_check.cpp (layouts, host bounds and the kernels' index arithmetic, under ASan + UBSan)."""
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hatch_ref as H
import mesh_slice_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(mesh_slice_ref.cases())
COS30 = (np.float32(np.cos(np.radians(30.0))), np.float32(np.sin(np.radians(30.0))))
DIRECTIONS = ((1.0, 0.0), (0.0, 1.0), COS30, (3.0, -4.0))
# (case, axis, line set of every layer, n_lines) -> (crossings, segments, odd lines or None)
KNOWN = [("box", 2, (1, 0, 0.5, 1), 12, (24, 12, 0)), ("box", 2, (0, 1, -11.5, 1), 12, (32, 16, None)),
         ("torus", 2, (1, 0, -10.25, 0.5), 64, (112, 56, None)), ("open_box", 0, (1, 0, 0.5, 1), 12, (8, 4, 0)),
         ("open_box", 0, (0, 1, -11.5, 1), 12, (6, 0, 6)), ("open_box", 0, (1, 1, -20.25, 0.5), 80, (28, 8, 12)),
         ("fin", 0, (1, 0, 0.5, 1), 12, (10, 4, 2)), ("fin", 2, (1, 0, 0.5, 1), 12, (12, 6, 0)),
         ("sphere", 1, (np.float32(0.8660254), 0.5, -30, 0.37), 200, (2922, 1461, 0))]


@pytest.fixture(scope="module")
def slices():
    return {(name, w): H.sliced(name, w) for name in NAMES for w in range(3)}


def covering_lines(result, n_layers, axis, d, n_target):
    """About n_target lines across the points' s range, a little beyond both ends."""
    u, v = (axis + 1) % 3, (axis + 2) % 3
    p = result["points"]
    s = H.normal_coordinate(p[:, u], p[:, v], np.float32(d[0]), np.float32(d[1])) if len(p) else np.array([0.0, 1.0])
    spacing = np.float32((s.max() - s.min()) / n_target)
    return H.as_lines((d[0], d[1], np.float32(s.min() - 1.25 * float(spacing)), spacing), n_layers), n_target + 4


def run(slices, name, w, line, n_lines, fn=H.hatch, zigzag=False):
    r, nl = slices[name, w]
    return fn(r["points"], r["contours"], nl, w, H.as_lines(line, nl), n_lines, zigzag)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("w", range(3))
def test_restatements_agree(slices, name, w):
    r, nl = slices[name, w]
    for d in DIRECTIONS:
        lines, n_lines = covering_lines(r, nl, w, d, 24)
        for zigzag in (False, True):
            a = H.hatch(r["points"], r["contours"], nl, w, lines, n_lines, zigzag)
            b = H.hatch_by_walk(r["points"], r["contours"], nl, w, lines, n_lines, zigzag)
            assert H.same(a, b), (d, zigzag, a["counts"], b["counts"])
            assert a["counts"]["crossings"] > 0 and a["segments"].dtype == b["segments"].dtype == np.float32


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: "%s-%d-%g-%g" % (c[0], c[1], c[2][0], c[2][1]))
def test_known_answers(slices, case):
    name, w, line, n_lines, (crossings, segments, odd) = case
    a, b = run(slices, name, w, line, n_lines), run(slices, name, w, line, n_lines, H.hatch_by_walk)
    assert H.same(a, b)
    c = a["counts"]
    assert (c["crossings"], c["segments"]) == (crossings, segments) and (odd is None or c["odd_lines"] == odd)


def test_box_torus_and_sphere_figures(slices):
    a = run(slices, "box", 2, (1, 0, 0.5, 1), 12)
    assert a["layer_first"].tolist() == [0, 0, 6, 12, 12] and H.lengths(a, 1, 0).tolist() == [8.0] * 12     # 96 = 2 x area 48 / spacing
    assert float(H.lengths(run(slices, "box", 2, (0, 1, -11.5, 1), 12), 0, 1).sum()) == 96.0
    t = run(slices, "torus", 2, (1, 0, -10.25, 0.5), 64)
    assert t["counts"]["lines_hit"] == 38 and t["counts"]["segments"] - t["counts"]["lines_hit"] == 18       # 18 lines pass the hole
    r, _ = slices["torus", 2]
    area = sum(mesh_slice_ref.area(r, c, 2) for c in range(len(r["contours"])))
    assert abs(float(H.lengths(t, 1, 0).sum()) * 0.5 - 225.51996) < 1e-4 and abs(area - 225.51940) < 1e-4
    assert run(slices, "sphere", 1, (np.float32(0.8660254), 0.5, -30, 0.37), 200)["counts"]["lines_hit"] == 1461


def test_ties_keep_the_enumeration_order(slices):
    """Two crossings of one line at one point: on fin, w = 2, the open two-point contour ends on the box's outline at
    V = (10, 4.51171875), and along (1, 1) V is the end of the smaller s of both the fin's segment and the box's next one.  A
    line through V (offset = s(V)) crosses both there with t = 0: equal keys, which the stable sort leaves in enumeration order.
    (With the direction (1, 0) and the half-integer lines of the known-answer table the fin's segment is parallel to the lines
    and crosses nothing: that case has 12 crossings, 6 segments and NO tie in either restatement.)"""
    r, nl = slices["fin", 2]
    assert run(slices, "fin", 2, (1, 0, 0.5, 1), 12)["ties"] == 0
    V = r["points"][int(r["contours"][1][0]) + 1]
    assert V[:2].tolist() == [10.0, 4.51171875]
    line = (1, 1, float(V[1]) - float(V[0]), 1)
    a, b = run(slices, "fin", 2, line, 8), run(slices, "fin", 2, line, 8, H.hatch_by_walk)
    assert a["ties"] >= 1 and H.same(a, b)


@pytest.mark.parametrize("name", ["box", "torus", "sphere"])
def test_closed_outlines_give_even_lines_and_ends_on_their_lines(slices, name):
    for w in range(3):
        r, nl = slices[name, w]
        assert r["counts"]["open_contours"] == 0
        u, v = (w + 1) % 3, (w + 2) % 3
        m = float(np.abs(r["points"][:, [u, v]]).max())
        for d in DIRECTIONS:
            lines, n_lines = covering_lines(r, nl, w, d, 37)
            a = H.hatch(r["points"], r["contours"], nl, w, lines, n_lines)
            c = a["counts"]
            assert c["odd_lines"] == 0 and c["crossings"] == 2 * c["segments"] and c["segments"] >= c["lines_hit"] > 0
            # both ends of every segment lie on its line, within the bound hatch_ref.s_tolerance derives from items 2 and 6
            k, j = a["line"] // n_lines, a["line"] % n_lines
            cl = lines[k, 2].astype(np.float64) + j.astype(np.float64) * lines[k, 3].astype(np.float64)
            tol = H.s_tolerance(m, d[0], d[1])
            for e in (0, 2):
                s = H.normal_coordinate(a["segments"][:, e], a["segments"][:, e + 1], lines[k, 0], lines[k, 1])
                assert float(np.abs(s - cl).max()) <= tol, (w, d, float(np.abs(s - cl).max()), tol)
            assert np.all(np.diff(a["line"].astype(np.int64)) >= 0)
            assert np.array_equal(a["layer_first"], np.searchsorted(k, np.arange(nl + 1)))


@pytest.mark.parametrize("name,w,d,n", [("box", 2, (1.0, 0.0), 13), ("torus", 2, COS30, 41), ("sphere", 1, COS30, 9)])
def test_midpoints_are_inside(slices, name, w, d, n):
    """Even-odd in exact arithmetic.  A midpoint closer to the outline than the bound of the previous test (in s, over |d| ~ 1: a
    distance) is skipped and counted; more than 1 % skipped fails."""
    r, nl = slices[name, w]
    lines, n_lines = covering_lines(r, nl, w, d, n)
    a = H.hatch(r["points"], r["contours"], nl, w, lines, n_lines)
    tol = H.s_tolerance(float(np.abs(r["points"]).max()), d[0], d[1])
    skipped = 0
    for seg, L in zip(a["segments"], a["line"]):
        k = int(L) // n_lines
        mx, my = (Fraction(float(seg[0])) + Fraction(float(seg[2]))) / 2, (Fraction(float(seg[1])) + Fraction(float(seg[3]))) / 2
        if H.distance_to_outline(r["points"], r["contours"], k, w, float(mx), float(my)) < tol:
            skipped += 1
            continue
        assert H.inside_even_odd(r["points"], r["contours"], k, w, mx, my), (seg, L)
    print("%s: %d segments, %d skipped" % (name, len(a["segments"]), skipped))
    assert len(a["segments"]) >= 20 and skipped <= 0.01 * len(a["segments"])


@pytest.mark.parametrize("name,w", [("sphere", 1), ("torus", 2), ("open_box", 0)])
def test_zigzag_is_the_stated_permutation(slices, name, w):
    r, nl = slices[name, w]
    lines, n_lines = covering_lines(r, nl, w, (1.0, 1.0), 31)
    plain = H.hatch(r["points"], r["contours"], nl, w, lines, n_lines)
    zig = H.hatch(r["points"], r["contours"], nl, w, lines, n_lines, True)
    assert plain["counts"] == zig["counts"] and np.array_equal(plain["line"], zig["line"]) and np.array_equal(plain["layer_first"], zig["layer_first"])
    want = plain["segments"].copy()
    for L in np.unique(plain["line"]):
        if (int(L) % n_lines) % 2 == 1:
            at = np.flatnonzero(plain["line"] == L)
            want[at] = plain["segments"][at[::-1]][:, [2, 3, 0, 1]]
    assert np.array_equal(want.view(np.uint32), zig["segments"].view(np.uint32)) and not np.array_equal(want, plain["segments"])


# ---- slicer: hatch_lines, the files, the command line --------------------------------------------------------------------------------
def as_slices(name, w):
    from ray_marching_amd import slicer
    r, nl = H.sliced(name, w)
    return slicer.Slices(r["points"], r["contours"], r["layer_first"], mesh_slice_ref.cases()[name][2], w), r, nl


def as_hatch(r, nl, w, lines, n_lines, zigzag=False):
    from ray_marching_amd import slicer
    a = H.hatch(r["points"], r["contours"], nl, w, lines, n_lines, zigzag)
    return slicer.Hatch(a["segments"], a["line"], a["layer_first"], lines, n_lines, a["counts"], {})


def test_hatch_lines():
    from ray_marching_amd import slicer
    s, r, nl = as_slices("sphere", 1)
    for spacing, angle, rotate in ((0.37, 45.0, 90.0), (1.5, 0.0, 67.0), (0.05, -30.0, 0.0)):
        lines, n_lines = slicer.hatch_lines(s, spacing, angle, rotate)
        assert lines.shape == (nl, 4) and lines.dtype == np.float32 and np.all(lines[:, 3] == np.float32(spacing))
        d = lines[:, :2].astype(np.float64)
        assert float(np.abs(np.hypot(d[:, 0], d[:, 1]) - 1.0).max()) <= 2.0 ** -23             # a unit vector to binary32 rounding
        u, v = s.in_plane_axes
        for k in range(nl):
            sk = H.normal_coordinate(r["points"][:, u], r["points"][:, v], lines[k, 0], lines[k, 1])
            c = H.line_values(lines, k, n_lines)
            assert c[0] < sk.min() and sk.max() < c[-1], k                                      # strictly inside (c_0, c_last)
            if spacing == 1.5:                                                                  # (exact in binary32)
                assert (float(lines[k, 2]) / 1.5 - 0.5) % 1.0 == 0.0, k                         # anchored at the world origin
        a = H.hatch(r["points"], r["contours"], nl, 1, lines, n_lines)
        assert a["counts"]["odd_lines"] == 0 and a["counts"]["segments"] > 0
    lines, _ = slicer.hatch_lines(s, 0.37, 45.0, 90.0)
    # rotate = 90: the angle is reduced modulo 360, so layers k and k + 4 share every bit; k and k + 2 run in opposite directions
    assert np.array_equal(lines[:-4].view(np.uint32), lines[4:].view(np.uint32))
    assert np.all(lines[:-2, 0] * lines[2:, 0] < 0) and np.all(lines[:-2, 1] * lines[2:, 1] < 0)
    assert np.allclose(lines[:-2, :2], -lines[2:, :2], atol=2.0 ** -23, rtol=0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            slicer.hatch_lines(s, bad)


def test_files_without_a_hatch_are_unchanged_and_with_one_round_trip(tmp_path):
    from ray_marching_amd import slicer
    s, r, nl = as_slices("box", 2)
    lines, n_lines = slicer.hatch_lines(s, 0.75, 30.0, 67.0)
    h = as_hatch(r, nl, 2, lines, n_lines)
    assert [len(h.layer(k)) for k in range(nl)] == np.diff(h.layer_first.astype(np.int64)).tolist() and h.length(0) == 0.0
    assert abs(h.length(1) * 0.75 - 48.0) < 0.75 * 28.0 * 0.75                   # area 48, perimeter 28: within a spacing's strip
    for ext, writer in (("svg", slicer.write_svg), ("cli", slicer.write_cli)):
        plain, none, viaw, withh = (str(tmp_path / ("%s.%s" % (n, ext))) for n in ("plain", "none", "write", "hatch"))
        writer(s, plain)
        writer(s, none, hatch=None)
        slicer.write(s, viaw)
        slicer.write(s, withh, h)
        text = open(plain).read()
        assert open(none).read() == text and open(viaw).read() == text
        marked = open(withh).read().splitlines(keepends=True)
        mark = '<path fill="none"' if ext == "svg" else "$$HATCHES/"
        assert "".join(l for l in marked if not l.startswith(mark)) == text and sum(l.startswith(mark) for l in marked) == 2
    got = []
    for l in open(str(tmp_path / "hatch.cli")):
        if l.startswith("$$HATCHES/"):
            f = l.strip().split("/")[1].split(",")
            assert f[0] == "1" and int(f[1]) * 4 == len(f) - 2
            got.append(np.array([float(x) for x in f[2:]], dtype=np.float64).astype(np.float32).reshape(-1, 4))
    assert np.array_equal(np.concatenate(got).view(np.uint32), h.segments.view(np.uint32))
    nums = re.findall(r'<path fill="none" d="([^"]*)"', open(str(tmp_path / "hatch.svg")).read())
    back = np.array([float(x) for d in nums for x in re.findall(r"[-+0-9.e]+", d)], dtype=np.float64).astype(np.float32).reshape(-1, 4)
    assert np.array_equal(back.view(np.uint32), h.segments.view(np.uint32))
    with pytest.raises(ValueError):
        slicer.write_cli(as_slices("torus", 2)[0], str(tmp_path / "x.cli"), h)   # a hatch of other slices: 4 layers against 1


def test_command_line_refusals():
    from ray_marching_amd import slicer
    for argv in (["--zigzag", "--layer-height", "0.1", "out.svg"], ["--hatch-angle", "30", "--layer-height", "0.1", "out.svg"],
                 ["--hatch-rotate", "30", "--mesh", "part.stl", "--layer-height", "0.1", "out.svg"],
                 ["--hatch", "0", "--layer-height", "0.1", "out.svg"], ["--hatch", "-0.5", "--mesh", "part.stl", "--layer-height", "0.1", "out.svg"],
                 ["--hatch", "nan", "--layer-height", "0.1", "out.svg"], ["--hatch", "x", "--layer-height", "0.1", "out.svg"],
                 ["--fail-on", "odd_lines>0", "--layer-height", "0.1", "out.svg"],                       # no --hatch, no --mesh
                 ["--hatch", "0.5", "--fail-on", "volume>0", "--layer-height", "0.1", "out.svg"]):
        with pytest.raises(SystemExit):
            slicer.main(argv)
    assert slicer.hatch_count_keys(dict.fromkeys(H.COUNT_NAMES, 1)) == dict.fromkeys(("segments_in", "crossings", "hatch_segments", "lines_hit", "odd_lines"), 1)
    assert slicer.parse_gates("odd_lines>0", tuple(slicer.hatch_count_keys(dict.fromkeys(H.COUNT_NAMES)))) == [("odd_lines", ">", 0)]


def test_constants_of_the_three_faces():
    from ray_marching_amd import _ffi
    assert _ffi.HATCH_COUNT_NAMES == H.COUNT_NAMES and len(_ffi.HATCH_COUNT_NAMES) == _ffi.RM_HATCH_COUNTS
    assert len(_ffi.HATCH_STAT_NAMES) == _ffi.RM_HATCH_STATS and _ffi.HATCH_STAT_NAMES[-1] == "scratch_bytes"
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rm_abi.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    found = 0
    for body in re.findall(r"enum\s+rm_hatch[a-z]+\s*\{(.*?)\}", header, re.S):
        for name, value in re.findall(r"(RM_HATCH_[A-Z_]+)\s*=\s*(\d+)", body):
            assert getattr(_ffi, name) == int(value), name
            assert re.search(r"pub const %s: c_int = %s;" % (name, value), rust), name
            found += 1
    assert found == 1 + 6 + 3
    for i, n in enumerate(_ffi.HATCH_COUNT_NAMES):
        assert getattr(_ffi, "RM_HATCH_" + n.upper()) == i
    assert "int rm_hatch_slices(" in header and "int rm_read_hatch(" in header


# ---- layouts, host bounds and index arithmetic, stand-alone under the sanitizers ------------------------------------------------------
def test_layout_check_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.fail("no C++ compiler")
    exe = str(tmp_path / "hatch_layout_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "ray-marching_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "hatch_layout_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
