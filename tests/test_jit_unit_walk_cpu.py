"""The single-unit path of the generated march kernel (csrc/rm_jit.h "Single-unit steps", RM_JIT_UNIT_WALK), the part that needs
no GPU: which programs get it, that the kernel compiles with and without it and keeps its registers, and that the
generator's classification of every unit -- a constant, the raw leaf value, the leaf value through the operators it still meets --
is what tests/unit_walk_ref.py's fold of the program with every other unit skipped gives, NaN, infinities and -0 included."""
import os
import re

import numpy as np
import pytest

import scenes
import unit_walk_ref as R
from ray_marching_amd import _ffi, renderer


def _mix():
    """every lattice operator and every bounded leaf kind in one chain: ((S - C) n B) u C u S"""
    t = scenes._Tab()
    a = t.op(scenes.SUBTRACTION, t.sphere((0, 0, 0), 1.0), t.cylinder((0.4, 0.0, 0.2), 0.3, 1.2))
    a = t.op(scenes.INTERSECTION, a, t.box((0, 0, 0), (0.9, 0.7, 0.9)))
    a = t.op(scenes.UNION, a, t.cylinder((1.6, 0.0, 0.0), 0.4, 0.5))
    return t.nodes, t.op(scenes.UNION, a, t.sphere((-1.5, 0.2, 0.0), 0.45))


def _leaves_then_operators():
    """S0 - (B1 n (S2 u C3)): four pushed leaves, then the operators on named values (the generator's folds of two operands)"""
    t = scenes._Tab()
    inner = t.op(scenes.UNION, t.sphere((0.5, 0, 0), 0.4), t.cylinder((0.0, 0.0, 0.5), 0.3, 0.6))
    return t.nodes, t.op(scenes.SUBTRACTION, t.sphere((0, 0, 0), 1.0), t.op(scenes.INTERSECTION, t.box((0.3, 0, 0), (0.5, 0.5, 0.5)), inner))


PROGRAMS = {
    "g32": scenes.g32, "g32_balanced": scenes.g32_balanced, "g8": scenes.g8, "g64": scenes.g64, "g8x": scenes.g8x,
    "mix": _mix, "right_deep6": lambda: scenes.right_deep(6), "leaves_then_operators": _leaves_then_operators,
}
# chains of at most 32 units (g64: 32 leaves), and trees whose units are their first records, get the path; the rest keep the
# straight-line code alone
WITH_PATH = {"g32": True, "g32_balanced": False, "g8": True, "g64": True, "g8x": True, "mix": True, "right_deep6": True,
             "leaves_then_operators": True}


def program(oracle, name):
    cc, w = oracle.serialize(*PROGRAMS[name]())
    return cc, np.asarray(w, dtype=np.uint32)


def source(cc, w, knob=None, prune=True):
    return renderer.jit_source(cc, w, prune=prune, env=None if knob is None else {"RM_JIT_UNIT_WALK": str(knob)})


def vgprs(code_object):
    """.vgpr_count of the (one) kernel in a code object's metadata note (msgpack: the key, then an unsigned integer)"""
    k = code_object.index(b".vgpr_count") + len(b".vgpr_count")
    v = code_object[k]
    return v if v < 0x80 else code_object[k + 1] if v == 0xCC else int.from_bytes(code_object[k + 1:k + 3], "big")


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_which_programs_get_the_path_and_the_knob_is_in_the_source(oracle, name):
    cc, w = program(oracle, name)
    default, off, on = source(cc, w), source(cc, w, 0), source(cc, w, 1)
    assert default == on                                        # the default is the path
    assert ("#define RM_JIT_UNIT_WALK 1" in on) == WITH_PATH[name] == (R.walk_body(on) is not None)
    assert "map_scene_walk" not in off and "RM_JIT_UNIT_WALK" not in off
    assert (off != on) == WITH_PATH[name]                       # the disk cache is keyed by the source: one kernel per setting
    # the straight-line function is the same text with and without the path in front of it
    body = lambda s: re.search(r"float map_scene_spec\(.*?\n\}\n", s, re.S).group(0)
    assert body(off) == body(on)
    # only pruned lattice kernels have it
    assert "map_scene_walk" not in source(cc, w, 1, prune=False)


@pytest.mark.parametrize("knob", [0, 1, 2])
@pytest.mark.parametrize("name", ["g32", "g32_balanced", "g8", "g64", "g8x"])
def test_the_kernel_compiles_and_g32_keeps_72_registers(oracle, name, knob, monkeypatch, tmp_path):
    cc, w = program(oracle, name)
    monkeypatch.setenv("RM_JIT_UNIT_WALK", str(knob))
    monkeypatch.setenv("RM_JIT_CACHE_DIR", "off")               # (a kernel read from the disk cache is not dumped)
    monkeypatch.setenv("RM_JIT_DUMP_DIR", str(tmp_path))
    rc, ms, nbytes, log = renderer.jit_compile(cc, w, prune=True)
    if rc != _ffi.RM_OK and "could not be loaded" in log:
        pytest.skip("libhiprtc is not installed: " + log)
    assert rc == _ffi.RM_OK, log
    assert nbytes > 4096
    if name == "g32":                                           # 7 waves per SIMD: 512 / 7 = 73.1 -> 72 registers
        co = [f for f in os.listdir(tmp_path) if f.endswith(".co")]
        assert len(co) == 1
        n = vgprs((tmp_path / co[0]).read_bytes())
        print("g32, RM_JIT_UNIT_WALK=%d: %d vector registers" % (knob, n))
        assert n <= 72


@pytest.mark.parametrize("name", sorted(n for n in PROGRAMS if WITH_PATH[n]))
def test_every_unit_is_classified_as_the_fold_with_the_others_skipped(oracle, name):
    cc, w = program(oracle, name)
    classes = R.walk_classes(source(cc, w, 1))
    kinds = R.leaf_kinds(cc, w)
    assert classes and len(kinds) <= 32
    covered = 0
    for mask, kind, expr in classes:
        covered |= (1 << len(kinds)) - 1 if mask is None else mask
    assert covered == (1 << len(kinds)) - 1 or classes[-1][0] is not None      # every unit has a class, or the rest takes the straight-line code
    evaluated = 0
    for u, leaf_kind in enumerate(kinds):
        c = R.class_of(classes, u)
        if c is None:
            continue
        kind, expr = c
        assert kind in (None, leaf_kind), "%s unit %d: a %s evaluated as a %s" % (name, u, leaf_kind, kind)
        evaluated += kind is not None
        for x in R.PROBES:
            want = R.fold_one_unit(cc, w, u, x)
            got = R.evaluate(expr, x)
            assert R.same_bits(got, want), "%s unit %d (%s), leaf value %r: %r from '%s', the fold gives %r" % (name, u, leaf_kind, x, got, expr, want)
            if kind is None:                                    # a constant: nothing is evaluated, whatever the leaf is
                assert "X" not in expr
            if not np.isnan(x):                                 # for numbers, skipping is the fold with the other leaves at +inf
                assert R.same_bits(want, R.fold_at_inf(cc, w, u, x)), (name, u, x)
    assert evaluated >= 1


def test_the_classes_of_the_metric_scene(oracle):
    """g32: record 0 is pushed (its raw value: a NaN stays a NaN through the skipped Unions behind it), the Unions meet an
    accumulator of +inf (v_min_f32 with +inf: a NaN leaf comes out as +inf), a subtracted leaf leaves +inf: no evaluation."""
    cc, w = program(oracle, "g32")
    classes = R.walk_classes(source(cc, w, 1))
    kinds = R.leaf_kinds(cc, w)
    by_unit = [R.class_of(classes, u) for u in range(16)]
    assert by_unit[0] == ("sphere", "X")
    for u in range(1, 16):
        if u % 4 == 0:
            assert by_unit[u] == (None, "inf")
        else:
            assert by_unit[u] == (kinds[u], "vmin_pinf(X)")
    nan = R.F(np.nan)
    assert np.isnan(R.fold_one_unit(cc, w, 0, nan)) and R.fold_one_unit(cc, w, 1, nan) == R.INF
    assert R.fold_at_inf(cc, w, 0, nan) == R.INF                 # (where the fold at +inf and the skipping code part)
