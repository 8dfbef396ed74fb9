"""Scene queries (rm_query_points / rm_cast_rays / rm_camera_rays) without a GPU: the symbols, the NULL-context contract,
the constants of the C header against the Rust and Python bindings, the Rust wrappers' slice checks, the Python methods,
and the query program the decoder builds (tests/test_gpu_query.py runs the queries themselves)."""
import ctypes as C
import os
import re

import numpy as np

import scenes
from ray_marching_amd import _ffi, renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY_FUNCTIONS = ("rm_query_points", "rm_cast_rays", "rm_camera_rays")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rm_abi.h")).read(), flags=re.S)


def rust_text():
    return open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()


def test_query_symbols_are_declared_and_exported():
    text = header_text()
    L = _ffi.hip_lib()
    for name in QUERY_FUNCTIONS:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert hasattr(L, name), "librm_hip.so does not export %s" % name


def test_null_context_is_an_error_not_a_crash():
    L = _ffi.hip_lib()
    xyz = np.zeros((4, 3), dtype=np.float32)
    out = np.zeros(64, dtype=np.float32)
    ids = np.zeros(64, dtype=np.uint32)
    assert L.rm_query_points(None, 4, xyz.ctypes.data, out.ctypes.data, None, ids.ctypes.data, 0, None) == _ffi.RM_ERR_NULL
    assert L.rm_cast_rays(None, 4, out.ctypes.data, out.ctypes.data, ids.ctypes.data, None, 0, None) == _ffi.RM_ERR_NULL
    assert L.rm_camera_rays(None, 8, 8, 0, 0, 2, 2, _ffi.RM_SAMPLE_CENTER, out.ctypes.data, 0, None) == _ffi.RM_ERR_NULL
    assert L.rm_query_points(None, 0, None, None, None, None, 0, None) == _ffi.RM_ERR_NULL


def test_constants_agree_between_header_rust_and_python():
    text = header_text()
    assert re.search(r"#define RM_NO_ID 0xFFFFFFFFu", text)
    assert re.search(r"#define RM_ABI_VERSION 2\b", text)      # the change is additive
    consts = {}
    for enum in ("rm_hit", "rm_sample"):
        body = re.search(r"enum\s+%s\s*\{(.*?)\}" % enum, text, re.S).group(1)
        consts.update({n: int(v) for n, v in re.findall(r"(RM_[A-Z0-9_]+)\s*=\s*(-?\d+)", body)})
    assert consts == {"RM_HIT_NONE": 0, "RM_HIT_SURFACE": 1, "RM_HIT_FLOOR": 2, "RM_SAMPLE_CENTER": 16}
    rust = dict(re.findall(r"pub const (RM_[A-Z0-9_]+): c_int = (-?\d+);", rust_text()))
    for name, value in consts.items():
        assert int(rust[name]) == value, name
        assert getattr(_ffi, name) == value, name
    assert re.search(r"pub const RM_NO_ID: u32 = 0xFFFF_?FFFF;", rust_text())
    assert _ffi.RM_NO_ID == 0xFFFFFFFF


def test_rust_wrappers_assert_slice_lengths_before_passing_pointers():
    src = rust_text()
    for name in ("query_points", "cast_rays", "camera_rays", "pick"):
        m = re.search(r"    pub fn %s\(&self(.*?)\n    \}\n" % name, src, re.S)
        assert m, "lib.rs has no wrapper RayMarchingResources::%s" % name
        body = m.group(1)
        if name == "pick":      # builds on the two checked wrappers, with arrays sized for one ray
            assert "self.camera_rays(" in body and "self.cast_rays(" in body and "as_ptr" not in body
            continue
        first_ptr = min(body.index(p) for p in ("as_ptr()", "as_mut_ptr()") if p in body)
        before = body[:first_ptr]
        slices = re.findall(r"(\w+): (?:Option<)?&(?:mut )?\[(?:f32|u32)\]", body.split("{", 1)[0])
        assert slices, name
        for s in slices:
            assert re.search(r"assert!\([^;]*\b%s\b[^;]*len\(\)" % s, before), "%s: no assert! on the length of %s before its pointer" % (name, s)
    assert re.search(r"pub struct Hit \{", src)


def test_python_methods_exist():
    for name in ("query_points", "cast_rays", "camera_rays", "pick", "query_points_device", "cast_rays_device",
                 "camera_rays_device"):
        assert callable(getattr(renderer.RayMarchingResources, name, None)), name


def _tag_every_leaf(cc, words):
    """Insert Material(ordinal) after every primitive: (cmd_count, words)."""
    nparam = {0: 4, 1: 6, 2: 4, 10: 5, 100: 0, 101: 0, 102: 0, 110: 1, 200: 3, 201: 0, 202: 4, 203: 0, 204: 1, 205: 0, 300: 1}
    w = [int(x) for x in words]
    out, q, k = [], 0, 0
    for _ in range(cc):
        op = w[q]
        out += w[q:q + 1 + nparam[op]]
        q += 1 + nparam[op]
        if op in (0, 1, 2, 10):
            out += [300, k % 256]
            k += 1
    return cc + k, np.asarray(out, dtype=np.uint32)


def test_program_facts_do_not_change_with_the_query_program(oracle):
    """A regression guard, not a test of new behaviour (it passes without the query program too): the decoder now builds a
    fourth decoding of every program, and rm_program_info must come out as before -- for a tagged program, the facts of its
    untagged form."""
    for name, f in list(scenes.SCENES.items()) + list(scenes.EXT_SCENES.items()):
        cc, w = oracle.serialize(*f())
        tc, tw = _tag_every_leaf(cc, w)
        assert renderer.program_info(tc, tw) == renderer.program_info(cc, w), name


def test_numpy_inputs_must_have_the_query_width():
    """The numpy path takes (n, width) arrays -- or one row of `width` -- and refuses any other shape instead of reading it
    as rows of `width` (an (n, 6) ray array passed as points would otherwise be 2n points).  No GPU needed: the shape is
    checked before the library is called."""
    import pytest
    check = renderer.RayMarchingResources._query_input
    kind, arr, n = check(None, np.zeros((5, 3)), 3, "points")
    assert kind == "numpy" and arr.dtype == np.float32 and arr.flags.c_contiguous and n == 5
    assert check(None, np.zeros(6), 6, "rays")[2] == 1
    for bad, width in ((np.zeros((4, 6)), 3), (np.zeros(12), 3), (np.zeros((2, 3)), 6), (np.zeros((2, 2, 3)), 3)):
        with pytest.raises(ValueError):
            check(None, bad, width, "x")
