"""The G-buffer draw without a GPU: the symbols and constants of the new entry points, rm_program_subtree against a Python
restatement, tests/gbuffer_ref.py (the numpy statement of DESIGN.md section 14 the GPU tests compare with) against the C
oracle's frame and counters, and the selection overlay."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gbuffer_ref
import scenes
from ray_marching_amd import _ffi, renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ALL_SCENES = dict(list(scenes.SCENES.items()) + list(scenes.EXT_SCENES.items()) + list(scenes.MAT_SCENES.items()))
NPARAM = gbuffer_ref.NPARAM
PUSHES, POPS, BINARY = (200, 202, 204), (201, 203, 205), (100, 101, 102, 110)


# ---- symbols and constants ----------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rm_abi.h")).read(), flags=re.S)
    L = _ffi.hip_lib()
    for name in ("rm_draw_gbuffer", "rm_program_subtree"):
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert hasattr(L, name), name
    assert re.search(r"#define RM_ABI_VERSION 2\b", header) and L.rm_abi_version() == 2


def test_sample_all_agrees_everywhere():
    header = open(os.path.join(ROOT, "include", "rm_abi.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    h = int(re.search(r"RM_SAMPLE_ALL\s*=\s*(\d+)", header).group(1))
    r = int(re.search(r"pub const RM_SAMPLE_ALL: c_int = (\d+);", rust).group(1))
    assert h == r == _ffi.RM_SAMPLE_ALL == gbuffer_ref.RM_SAMPLE_ALL == 17
    assert _ffi.RM_SAMPLE_CENTER == gbuffer_ref.RM_SAMPLE_CENTER == 16
    for fn in ("rm_draw_gbuffer", "rm_program_subtree"):
        assert re.search(r"pub fn %s\(" % fn, rust), fn
    for wrapper in ("pub fn draw_gbuffer(&self", "pub fn program_subtree("):
        assert wrapper in rust, wrapper


def test_python_methods_exist():
    for name in ("draw_gbuffer", "draw_gbuffer_device"):
        assert callable(getattr(renderer.RayMarchingResources, name))
    assert callable(renderer.program_subtree) and callable(renderer.selection_overlay)
    assert renderer.RayMarchingResources.GBUFFER_KEYS == gbuffer_ref.KEYS


def test_null_context_is_an_error_not_a_crash():
    out = np.zeros(64, dtype=np.uint32)
    L = _ffi.hip_lib()
    assert L.rm_draw_gbuffer(None, 4, 4, 0, 4, _ffi.RM_SAMPLE_ALL, 0, 0, None, out.ctypes.data, None, 0, None) == _ffi.RM_ERR_NULL
    assert L.rm_draw_gbuffer(None, 4, 4, 0, 4, _ffi.RM_SAMPLE_ALL, 0, 0, None, None, None, 0, None) == _ffi.RM_ERR_NULL


# ---- rm_program_subtree -------------------------------------------------------------------------------------------------------
def subtree_restated(cc, words):
    """(first, count) for every command index: a value stack of first commands, a stack of open Pushes."""
    w = [int(x) for x in words]
    out, values, pushes, q = [None] * cc, [], [], 0
    for i in range(cc):
        op = w[q]
        q += 1 + NPARAM[op]
        if op in PUSHES:
            pushes.append(i)
            continue
        if op in POPS:
            values[-1] = pushes.pop()
            out[values[-1]] = (values[-1], i - values[-1] + 1)       # the Push: the range of its Pop
        elif op in BINARY:
            values.pop()
        elif op != 300:
            values.append(i)
        out[i] = (values[-1], i - values[-1] + 1)
    return out


def random_words(rng, depth):
    """A random valid postfix program with transforms and tags -> (cmd_count, list of words)."""
    f = lambda *v: [int(x) for x in np.asarray(v, F).view(np.uint32)]   # noqa: E731
    r = rng.random()
    if depth == 0 or r < 0.25:
        k = int(rng.integers(0, 4))
        c = rng.uniform(-2, 2, 3)
        if k == 0:
            return 1, [0] + f(*c, rng.uniform(0.1, 0.8))
        if k == 1:
            return 1, [1] + f(*c, *rng.uniform(0.1, 0.6, 3))
        if k == 2:
            return 1, [10] + f(*c, 0.3, 0.5)
        return 1, [2] + f(0.0, 1.0, 0.0, 1.0)
    if r < 0.45:
        n, w = random_words(rng, depth - 1)
        k = int(rng.integers(0, 3))
        push = [[200] + f(*rng.uniform(-1, 1, 3)), [202] + f(1.0, 0.0, 0.0, 0.0), [204] + f(rng.uniform(0.5, 2.0))][k]
        return n + 2, push + w + [201 + 2 * k]
    if r < 0.6:
        n, w = random_words(rng, depth - 1)
        return n + 1, w + [300, int(rng.integers(0, 6))]
    na, wa = random_words(rng, depth - 1)
    nb, wb = random_words(rng, depth - 1)
    op = int(rng.choice(BINARY))
    return na + nb + 1, wa + wb + ([op] + f(0.3) if op == 110 else [op])


def opcodes(words, cc):
    out, q = [], 0
    for _ in range(cc):
        out.append(int(words[q]))
        q += 1 + NPARAM[int(words[q])]
    return out


def subtree_programs(oracle):
    progs = [(name, *oracle.serialize(*fn())) for name, fn in sorted(ALL_SCENES.items())]
    progs.append(("right_deep(32)", *oracle.serialize(*scenes.right_deep(32))))
    rng = np.random.default_rng(14)
    for k in range(300):
        progs.append(("random %d" % k, *random_words(rng, int(rng.integers(1, 6)))))
    return progs


def test_subtree_equals_the_stack_restatement(oracle):
    kinds = set()
    for name, cc, w in subtree_programs(oracle):
        w = np.asarray(w, dtype=np.uint32)
        assert renderer.validate_program(cc, w)[0] == _ffi.RM_OK, name
        want = subtree_restated(cc, w)
        got = [renderer.program_subtree(cc, w, i) for i in range(cc)]
        assert got == want, name
        assert got[cc - 1] == (0, cc), name           # the root
        ops = opcodes(w, cc)
        kinds |= set(ops)
        for i, op in enumerate(ops):
            first, count = got[i]
            assert first <= i < first + count <= cc
            if op in gbuffer_ref.PRIMS:
                assert got[i] == (i, 1)
            elif op in POPS:
                assert ops[first] == op - 1 and got[first] == got[i]     # a Push and its Pop give the same range
    assert kinds >= {0, 1, 100, 101, 102, 110, 200, 201, 202, 203, 204, 205, 300}


def test_subtree_errors(oracle):
    L = _ffi.hip_lib()
    u32p = C.POINTER(C.c_uint32)
    first, count = C.c_uint32(7), C.c_uint32(7)
    cc, w = oracle.serialize(*scenes.g8())
    w = np.ascontiguousarray(w, dtype=np.uint32)
    for index in (cc, cc + 1, 0xFFFFFFFF):
        assert L.rm_program_subtree(cc, w.ctypes.data_as(u32p), len(w), index, C.byref(first), C.byref(count)) == _ffi.RM_ERR_RANGE
        with pytest.raises(_ffi.RmError) as e:
            renderer.program_subtree(cc, w, index)
        assert e.value.status == _ffi.RM_ERR_RANGE
    assert L.rm_program_subtree(0, None, 0, 0, C.byref(first), C.byref(count)) == _ffi.RM_ERR_RANGE      # the empty program
    assert (first.value, count.value) == (7, 7)       # a failed call writes nothing
    assert L.rm_program_subtree(cc, w.ctypes.data_as(u32p), len(w), 0, None, None) == _ffi.RM_OK       # outputs are optional
    bad = [("truncated sphere", 1, [0, 0, 0]), ("operator on empty stack", 1, [100]),
           ("operator with one operand", 2, [0, 0, 0, 0, 0x3F800000, 101]), ("unknown opcode", 1, [7]),
           ("cmd_count beyond words", 3, [0, 0, 0, 0, 0x3F800000]), ("pop without push", 2, [0, 0, 0, 0, 0x3F800000, 201]),
           ("push left open", 2, [200, 0, 0, 0, 0, 0, 0, 0, 0x3F800000]), ("tag on nothing", 1, [300, 1])]
    for label, n, words in bad:
        rc = renderer.validate_program(n, words)[0]
        assert rc < 0, label
        a = np.asarray(words, dtype=np.uint32)
        assert L.rm_program_subtree(n, a.ctypes.data_as(u32p), len(a), 0, C.byref(first), C.byref(count)) == rc, label


# ---- gbuffer_ref against the C oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g32", "mat_mix"])
def test_reference_agrees_with_the_oracle_frame(oracle, name):
    W, H = 64, 48
    lim = (0.01, 100.0, 128)
    cc, w = oracle.serialize(*ALL_SCENES[name]())
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    ud = {"viewport_extent": list(u.viewport_extent), "inv_proj": list(u.inv_proj), "inv_view": list(u.inv_view)}
    mats = scenes.MATERIAL_TABLE if name in scenes.MAT_SCENES else None
    img, cnt = oracle.render(u, lim, cc, w, W, H, threads=4, want_counters=True, materials=mats)
    g = gbuffer_ref.render(ud, lim, cc, w, W, H)
    black = np.all(img[..., :3] == 0, axis=-1)
    nothing = (g["surface_mask"] == 0) & (g["floor_mask"] == 0)
    assert np.array_equal(black, nothing)
    assert black.any() and not black.all()
    assert int(g["steps"].astype(np.uint64).sum()) == cnt["march_steps"]
    # what the records promise about themselves
    assert np.all((g["surface_mask"] & g["floor_mask"]) == 0) and np.all((g["surface_mask"] | g["floor_mask"]) < 65536)
    assert np.all((g["kind"] == gbuffer_ref.RM_HIT_NONE) == nothing) and np.all(np.isinf(g["t"]) == nothing)
    assert np.all(g["sample"][nothing] == gbuffer_ref.RM_NO_ID) and np.all(g["sample"][~nothing] < 16)
    hit = (g["surface_mask"] | g["floor_mask"])[~nothing]
    assert np.all((hit >> g["sample"][~nothing]) & 1 == 1)            # the nearest sample is one of the samples that hit
    surf = g["kind"] == gbuffer_ref.RM_HIT_SURFACE
    assert np.all(g["leaf"][~surf] == gbuffer_ref.RM_NO_ID) and np.all(g["leaf"][surf] < cc)
    assert not np.isnan(g["t"]).any()


# ---- the overlay ---------------------------------------------------------------------------------------------------------------
def test_selection_overlay_on_a_hand_made_mask():
    img = np.zeros((2, 3, 4), dtype=F)
    img[..., :3] = 0.5
    img[..., 3] = 1.0
    mask = np.array([[0x0000, 0xFFFF, 0x00FF], [0x0001, 0x8000, 0xF0F0]], dtype=np.uint32)
    out = renderer.selection_overlay(img, mask, 16, (1.0, 0.0, 0.0), alpha=1.0)
    assert out.dtype == F and out.shape == img.shape and np.all(out[..., 3] == 1.0) and np.all(img[..., :3] == 0.5)
    cover = np.array([[0, 16, 8], [1, 1, 8]], dtype=F) / F(16)
    assert np.array_equal(out[..., 0], F(0.5) * (F(1) - cover) + cover)
    assert np.array_equal(out[..., 1], F(0.5) * (F(1) - cover)) and np.array_equal(out[..., 2], out[..., 1])
    half = renderer.selection_overlay(img, mask, 16, (1.0, 0.0, 0.0), alpha=0.5)
    assert np.array_equal(half[..., 0], F(0.5) * (F(1) - F(0.5) * cover) + F(0.5) * cover)
    one = renderer.selection_overlay(img, np.array([[0, 1 << 16, 0], [1 << 9, 0, 0]], dtype=np.uint32), 1, (0.0, 1.0, 0.0), alpha=1.0)
    assert np.array_equal(one[..., 1], np.array([[0.5, 1.0, 0.5], [1.0, 0.5, 0.5]], dtype=F))
    with pytest.raises(ValueError):
        renderer.selection_overlay(img, mask[:1], 16, (1, 0, 0))
